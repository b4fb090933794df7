"""Psychoacoustic masking model on MI355X.

Drop-in for ``audiocodec.psychoacoustic.PsychoacousticModel`` (reference
``audiocodec/psychoacoustic.py:13-339``): same constructor keywords, methods, layouts and
attributes, on ``torch`` ROCm tensors.  Constants are pre-computed in float64 by the native
library (host side), the per-frame model runs in hand-written HIP kernels.
"""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import torch

from . import _host, _lib, placement


class _TonalityFn(torch.autograd.Function):
    """Differentiable ``tonality`` (the reference is differentiated by TensorFlow inside a training graph,
    ``psychoacoustic.py:311``); the backward pass is the explicit adjoint kernel ``ac_tonality_backward``.  Like every
    backward here it runs kernels autograd cannot see, so it is marked ``once_differentiable``: a second-order backward
    raises instead of silently dropping their part (the gradient of ``add_noise`` w.r.t. ``thr`` among them)."""

    @staticmethod
    def forward(ctx, X, model):
        ctx.model = model
        ctx.save_for_backward(X)
        return model._tonality(X)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gt):
        (X,) = ctx.saved_tensors
        return ctx.model._tonality_backward(X, gt.contiguous()), None


class _ThresholdFn(torch.autograd.Function):
    """Differentiable ``global_masking_threshold`` w.r.t. the amplitudes and the tonality (``ac_mask_threshold_backward``)."""

    @staticmethod
    def forward(ctx, X, t, model, drown):
        ctx.model, ctx.drown = model, drown
        ctx.save_for_backward(X, t)
        return model._threshold(X, t, drown)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gthr):
        X, t = ctx.saved_tensors
        gX, gt = ctx.model._threshold_backward(X, t, ctx.drown, gthr.contiguous())
        return gX, gt, None, None


class _AddNoiseFn(torch.autograd.Function):
    """Differentiable ``add_noise`` (a plain differentiable op chain in the reference, ``psychoacoustic.py:150-167``):
    out = X + thr * n with n ~ Normal(0, 1/6) fixed by the seed, so d out / d X = 1 and d out / d thr = n; the second is
    the same kernel run on (0, grad_out) under the same seed."""

    @staticmethod
    def forward(ctx, X, thr, model, seed):
        ctx.model, ctx.seed = model, seed
        return model._add_noise(X, thr, seed)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        gX = g if ctx.needs_input_grad[0] else None
        gthr = ctx.model._add_noise(None, g, ctx.seed) if ctx.needs_input_grad[1] else None
        return gX, gthr, None, None


class _DbFn(torch.autograd.Function):
    """Differentiable ``amplitude_to_dB`` / ``amplitude_to_dB_norm`` (``psychoacoustic.py:71-100``): the adjoint kernel
    ``ac_amplitude_to_db_backward`` (zero inside the clamp at ``_INTENSITY_EPS``)."""

    @staticmethod
    def forward(ctx, a, model, norm):
        ctx.model, ctx.norm = model, norm
        ctx.save_for_backward(a)
        return model._elementwise_db(a, norm)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        return ctx.model._db_backward(a, g.contiguous(), ctx.norm), None, None


class PsychoacousticModel:
    SPREADING = {"f32": 0, "bf16_mfma": 1, "bf16x2_mfma": 2}

    def __init__(self, sample_rate, filter_bands_n=1024, bark_bands_n=64, alpha=0.6,
                 compute_dtype=torch.float32, precompute_dtype=torch.float64, spreading=None):
        """Same signature as the reference (``psychoacoustic.py:14-15``) plus one extension:

        :param spreading: form of the band x band product with the spreading matrix (``psychoacoustic.py:205-207``) in
                          the wave-level kernels (include/audiocodec_amd.h, AC_SPREAD_*): ``"f32"`` vector-ALU
                          multiply-adds, ``"bf16_mfma"`` bfloat16 operands on the matrix cores (thresholds within 5e-3),
                          ``"bf16x2_mfma"`` split-bfloat16 operands on the matrix cores (thresholds within the 1e-4
                          parity bar).  None = the library's default: ``"bf16x2_mfma"`` where the wave-level kernels
                          serve the model (filter_bands_n 1024 / 2048, 64 Bark bands), ``"f32"`` otherwise (the
                          AC_SPREAD tuning hook overrides).  Asking for a matrix-core form elsewhere is an error

        :raises TypeError: when compute_dtype is not float64, float32 or bfloat16 (``:42-43``).  float32 runs the
                           wave-level kernels; float64 runs float64 kernels on float64 constants (the on-device
                           cross-check); bfloat16 means bfloat16 tensors with float32 arithmetic inside.  Autograd is
                           float32 only
        """
        self.alpha = alpha
        self.sample_rate = sample_rate
        self.bark_bands_n = int(bark_bands_n)
        self.filter_bands_n = int(filter_bands_n)
        compute_dtype = _host.as_torch_dtype(compute_dtype)
        if compute_dtype not in (torch.float64, torch.float32, torch.bfloat16):
            raise TypeError("compute_dtype of PsychoacousticModel should be float64, float32 or bfloat16")
        self.compute_dtype = compute_dtype
        self._dtype_id = _host.require_hip_compute_dtype(compute_dtype, "PsychoacousticModel")
        self.precompute_dtype, self._pre_id = _host.precompute_id(precompute_dtype, "PsychoacousticModel")
        self._lib = _lib.load()

        N, M = self.filter_bands_n, self.bark_bands_n
        # constants computed in the precompute dtype (``:61-69``), then held in the compute dtype, as the reference holds
        # them (float64: unrounded; bfloat16: float32 here, the kernels' arithmetic type)
        np_t = np.float64 if compute_dtype == torch.float64 else np.float32
        W = np.empty((N, M), dtype=np.float64)
        W_inv = np.empty((M, N), dtype=np.float64)
        S = np.empty((M, M), dtype=np.float64)
        quiet = np.empty((M,), dtype=np.float64)
        scalars = np.empty((4,), dtype=np.float64)
        fp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self._lib.ac_psy_tables_host_pre(
            N, M, float(sample_rate), float(alpha), self._pre_id, W.ctypes.data_as(fp), W_inv.ctypes.data_as(fp),
            S.ctypes.data_as(fp), quiet.ctypes.data_as(fp), scalars.ctypes.data_as(fp)))
        W, W_inv, S, quiet = (v.astype(np_t) for v in (W, W_inv, S, quiet))
        self._dB_MAX = torch.tensor(120.0, dtype=compute_dtype)                 # :52
        self._INTENSITY_EPS = torch.tensor(1e-14, dtype=compute_dtype)          # :56
        self._dB_MIN = torch.tensor(scalars[3], dtype=compute_dtype)            # :58  (= -20 dB)
        self.max_frequency = torch.tensor(scalars[0], dtype=self.precompute_dtype)      # :61
        self.max_bark = torch.tensor(scalars[1], dtype=self.precompute_dtype)           # :62
        self.bark_band_width = torch.tensor(scalars[2], dtype=self.precompute_dtype)    # :63
        self.W = torch.from_numpy(W)                                            # :66
        self.W_inv = torch.from_numpy(W_inv)                                    # :67
        self.quiet_threshold_intensity = torch.from_numpy(quiet).reshape(1, 1, M, 1)   # :68
        self.spreading_matrix = torch.from_numpy(S)                             # :69

        sr, al, lib, pre = float(sample_rate), float(alpha), self._lib, self._pre_id
        if spreading is not None and spreading not in self.SPREADING:
            raise ValueError("spreading must be one of %s" % sorted(self.SPREADING))
        self.spreading = spreading
        mode = -1 if spreading is None else self.SPREADING[spreading]   # -1: the library's default for the plan
        create = lambda dev, out: lib.ac_psy_plan_create_pre(N, M, sr, al, dev, mode, pre, out)   # noqa: E731
        self._plans = _host.PlanCache(self, create, lib.ac_psy_plan_destroy)
        self._row_budget = None
        self._base = None
        self._band_ids = {}       # device -> the band of every bin (mix_to_budget); shared with the models made from this one

    def with_row_budget(self, row_bits, min_offset=0):
        """A model with the same constants whose plans carry a row budget (``ac_psy_plan_with_row_budget``; DESIGN.md
        section 8c): on it :meth:`quantize` gives the codes and scale factors of
        ``quantize_to_budget(X, thr, row_bits, min_offset)``, and a codec built around it encodes at that budget in its fused
        launch.  Everything else is unchanged, :meth:`quantize_to_budget` and :meth:`quantize_to_clip_budget` (which obey
        their own arguments) included.  Called on a budgeted model it replaces the budget.  ``row_bits``: an int, at least
        5 * bark_bands_n; ``min_offset`` in [-254, 254]; float32 only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        if isinstance(row_bits, bool) or not isinstance(row_bits, (int, np.integer)):
            raise TypeError("row_bits must be an int, got %s" % type(row_bits).__name__)
        if not 5 * self.bark_bands_n <= int(row_bits) <= 2 ** 31 - 1:
            raise ValueError("row_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band, or "
                             "above int32" % (row_bits, 5 * self.bark_bands_n))
        self._check_min_offset(min_offset)
        base = self._base if self._base is not None else self
        R, kmin, lib = int(row_bits), int(min_offset), self._lib
        new = copy.copy(base)
        new._base = base          # (the derived plans are built from the base model's: it stays alive with this one)
        new._row_budget = (R, kmin)
        create = lambda dev, out: lib.ac_psy_plan_with_row_budget(   # noqa: E731
            base._plans.get(torch.device("cuda", dev)), R, kmin, out)
        new._plans = _host.PlanCache(new, create, lib.ac_psy_plan_destroy)
        return new

    @property
    def row_budget(self):
        """``(row_bits, min_offset)`` of a model made by :meth:`with_row_budget`, else None."""
        return self._row_budget

    def _plan(self, device):
        return self._plans.get(device)

    def is_fast(self, device=None):
        dev = _host.default_device(device)
        return bool(self._lib.ac_psy_plan_is_fast(self._plans.get(dev)))

    def tier(self, device=None):
        """2: wave-level kernels fused into the encode; 1: wave-level kernels for general band layouts; 0: generic kernels
        (``ac_psy_plan_tier``)."""
        dev = _host.default_device(device)
        return int(self._lib.ac_psy_plan_tier(self._plans.get(dev)))

    def plan_spreading(self, device=None):
        """The form of the spreading product the plan on ``device`` runs (a key of ``SPREADING``)."""
        dev = _host.default_device(device)
        mode = self._lib.ac_psy_plan_spreading(self._plans.get(dev))
        return {v: k for k, v in self.SPREADING.items()}[mode]

    # ---- element-wise utilities -----------------------------------------------------------------
    def _elementwise_db(self, mdct_amplitude, norm):
        a = mdct_amplitude
        if not isinstance(a, torch.Tensor):
            raise TypeError("mdct_amplitude must be a torch.Tensor")
        if a.dtype != self.compute_dtype:
            raise ValueError("mdct_amplitude has dtype %s but compute_dtype is %s" % (a.dtype, self.compute_dtype))
        if not a.is_cuda:
            raise RuntimeError("mdct_amplitude lives on %s: no CPU fallback" % a.device)
        a = a.contiguous()
        out = torch.empty_like(a)
        with _host.on_device(a.device):
            _lib.check(self._lib.ac_amplitude_to_db_typed(_host.ptr(a), _host.ptr(out), a.numel(), int(norm),
                                                          self._dtype_id, _host.stream_ptr(a.device)))
        return out

    def _db_backward(self, a, g, norm):
        # the kernel walks three flat arrays in the logical (row-major) order: one contiguous copy of each input, held until
        # the launch has been enqueued, and a contiguous result (a permuted view would otherwise get a scrambled gradient)
        a_c, g_c = a.contiguous(), g.contiguous()
        ga = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        with _host.on_device(a.device):
            _lib.check(self._lib.ac_amplitude_to_db_backward(_host.ptr(a_c), _host.ptr(g_c), _host.ptr(ga),
                                                             a_c.numel(), int(norm), _host.stream_ptr(a.device)))
        return ga

    def _db(self, mdct_amplitude, norm):
        a = mdct_amplitude
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            _host.require_float32(self.compute_dtype, "the backward pass of amplitude_to_dB")
            return _DbFn.apply(a, self, norm)
        return self._elementwise_db(a, norm)

    def amplitude_to_dB(self, mdct_amplitude):
        """``amplitude_to_dB`` (``psychoacoustic.py:71-85``): [-1,1] amplitude -> dB in [_dB_MIN, _dB_MAX].
        Differentiable (float32)."""
        return self._db(mdct_amplitude, False)

    def amplitude_to_dB_norm(self, mdct_amplitude):
        """``amplitude_to_dB_norm`` (``psychoacoustic.py:87-100``): dB scale normalised to [0, 1].  Differentiable
        (float32)."""
        return self._db(mdct_amplitude, True)

    # ---- per-frame model -------------------------------------------------------------------------
    def _check_spectrum(self, X, name="mdct_amplitudes"):
        X = _host.check_device_tensor(X, name, self.compute_dtype, 4)
        if X.shape[2] != self.filter_bands_n:
            raise ValueError("axis 2 of %s (%d) != filter_bands_n (%d)" % (name, X.shape[2], self.filter_bands_n))
        return X

    def tonality(self, mdct_amplitudes):
        """``tonality`` (``psychoacoustic.py:102-120``): [B, K, N, C] -> [B, K, 1, C] in [0, 1]."""
        if isinstance(mdct_amplitudes, torch.Tensor) and mdct_amplitudes.requires_grad and torch.is_grad_enabled():
            return _TonalityFn.apply(mdct_amplitudes, self)   # (every compute_dtype: ac_tonality_backward_typed)
        return self._tonality(mdct_amplitudes)

    def _tonality(self, mdct_amplitudes):
        X = self._check_spectrum(mdct_amplitudes)
        B, F, N, C = X.shape
        t = torch.empty((B, F, 1, C), dtype=X.dtype, device=X.device)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_tonality_typed(self._plans.get(X.device), _host.ptr(X), _host.ptr(t),
                                                   self._dtype_id, B, F, C, _host.stream_ptr(X.device)))
        return t

    def _tonality_backward(self, X, gt):
        X = self._check_spectrum(X)
        B, F, N, C = X.shape
        gX = torch.empty_like(X)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_tonality_backward_typed(self._plans.get(X.device), _host.ptr(X), _host.ptr(gt), _host.ptr(gX),
                                                            self._dtype_id, B, F, C, _host.stream_ptr(X.device)))
        return gX

    def global_masking_threshold(self, mdct_amplitudes, tonality_per_block, drown=0.0):
        """``global_masking_threshold`` (``psychoacoustic.py:122-148``): -> [B, K, N, C], strictly positive."""
        needs_grad = any(isinstance(v, torch.Tensor) and v.requires_grad for v in (mdct_amplitudes, tonality_per_block))
        if needs_grad and torch.is_grad_enabled():
            return _ThresholdFn.apply(mdct_amplitudes, tonality_per_block, self, float(drown))
        return self._threshold(mdct_amplitudes, tonality_per_block, drown)

    def _threshold_backward(self, X, t, drown, gthr):
        X = self._check_spectrum(X)
        B, F, N, C = X.shape
        t = t.contiguous()
        gX = torch.empty_like(X)
        gt = torch.empty_like(t)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_mask_threshold_backward_typed(self._plans.get(X.device), _host.ptr(X), _host.ptr(t),
                                                                  float(drown), _host.ptr(gthr), _host.ptr(gX), _host.ptr(gt),
                                                                  self._dtype_id, B, F, C, _host.stream_ptr(X.device)))
        return gX, gt

    def _threshold(self, mdct_amplitudes, tonality_per_block, drown=0.0):
        X = self._check_spectrum(mdct_amplitudes)
        B, F, N, C = X.shape
        t = _host.check_device_tensor(tonality_per_block, "tonality_per_block", self.compute_dtype, 4)
        if tuple(t.shape) != (B, F, 1, C):
            raise ValueError("tonality_per_block must have shape %s, got %s" % ((B, F, 1, C), tuple(t.shape)))
        if t.device != X.device:
            raise ValueError("mdct_amplitudes and tonality_per_block live on different devices")
        thr = placement.empty(placement.REGION_OTHER, tuple(X.shape), X.dtype, X.device)   # (see placement.py)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_mask_threshold_typed(self._plans.get(X.device), _host.ptr(X), _host.ptr(t),
                                                         float(drown), _host.ptr(thr), self._dtype_id, B, F, C,
                                                         _host.stream_ptr(X.device)))
        return thr

    def add_noise(self, mdct_amplitudes, masking_threshold, seed=None):
        """``add_noise`` (``psychoacoustic.py:150-167``): X + thr * Normal(0, 1/6).

        The generator is counter-based (seed, element index); the stream differs from TensorFlow's, so
        parity is statistical (mean 0, sigma = thr / 6).  ``seed=None`` draws one from torch's generator.
        Differentiable with respect to both inputs (float32): the noise is a constant of the seed.
        """
        X = self._check_spectrum(mdct_amplitudes)
        thr = _host.check_device_tensor(masking_threshold, "masking_threshold", self.compute_dtype, 4)
        if thr.shape != X.shape or thr.device != X.device:
            raise ValueError("masking_threshold must match mdct_amplitudes in shape and device")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        seed = int(seed) & (2 ** 64 - 1)
        if (X.requires_grad or thr.requires_grad) and torch.is_grad_enabled():
            _host.require_float32(self.compute_dtype, "the backward pass of add_noise")
            return _AddNoiseFn.apply(X, thr, self, seed)
        return self._add_noise(X, thr, seed)

    def _add_noise(self, X, thr, seed):
        """X may be None (zeros): thr * Normal(0, 1/6) under the same seed."""
        out = torch.empty_like(thr)
        with _host.on_device(thr.device):
            _lib.check(self._lib.ac_add_noise_typed(_host.ptr(X) if X is not None else None, _host.ptr(thr), _host.ptr(out),
                                                    thr.numel(), seed, self._dtype_id, _host.stream_ptr(thr.device)))
        return out

    # ---- quantiser (extension: what add_noise stands in for) -----------------------
    @property
    def scale_band_offsets(self):
        """Scale-factor bands of the quantiser: int32 offsets ``[bark_bands_n + 1]``; band j holds bins
        ``[o[j], o[j+1])`` (``ac_psy_scale_bands_host``, computed on the host in float64, no GPU needed)."""
        off = np.empty((self.bark_bands_n + 1,), dtype=np.int32)
        _lib.check(self._lib.ac_psy_scale_bands_host(float(self.sample_rate), self.filter_bands_n, self.bark_bands_n,
                                                     off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return off

    def _check_quant_tensor(self, t, name, dtype, shape=None, device=None, ndim=4):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.requires_grad and torch.is_grad_enabled():
            raise ValueError("%s requires a gradient: quantisation is not differentiable -- use add_noise(), its "
                             "differentiable stand-in" % name)
        if t.dtype != dtype:
            raise ValueError("%s has dtype %s, expected %s" % (name, t.dtype, dtype))
        if t.dim() != ndim:
            raise ValueError("%s must have %d dimensions, got shape %s" % (name, ndim, tuple(t.shape)))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
        if not t.is_cuda:
            raise ValueError("%s lives on %s: the quantiser runs on ROCm device tensors only" % (name, t.device))
        if device is not None and t.device != device:
            raise ValueError("%s lives on %s but %s" % (name, t.device, device))
        t = t.contiguous()
        if t.data_ptr() % 16 != 0:      # a view that starts inside an allocation: the kernels want 16-byte aligned rows
            t = t.clone()
        return t

    def _check_quant_inputs(self, mdct_amplitudes, masking_threshold):
        """The checks every quantising method makes of X and thr [B, F, N, C] float32; returns them ready for the kernels."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        X = self._check_quant_tensor(mdct_amplitudes, "mdct_amplitudes", torch.float32)
        N = X.shape[2]
        if N != self.filter_bands_n:
            raise ValueError("axis 2 of mdct_amplitudes (%d) != filter_bands_n (%d)" % (N, self.filter_bands_n))
        thr = self._check_quant_tensor(masking_threshold, "masking_threshold", torch.float32, X.shape, X.device)
        return X, thr

    @staticmethod
    def _check_min_offset(min_offset):
        if isinstance(min_offset, bool) or not isinstance(min_offset, (int, np.integer)):
            raise TypeError("min_offset must be an int, got %s" % type(min_offset).__name__)
        if not -254 <= int(min_offset) <= 254:
            raise ValueError("min_offset (%d) outside [-254, 254]" % min_offset)

    def _alloc_codes(self, X, rate=False):
        """codes int16 [B, F, N, C] and sf int8 [B, F, M, C] for X; rate: also offset int16 and row bits int32 [B, F, C]."""
        B, F, N, C = X.shape
        out = (torch.empty((B, F, N, C), dtype=torch.int16, device=X.device),
               torch.empty((B, F, self.bark_bands_n, C), dtype=torch.int8, device=X.device))
        if rate:
            out += (torch.empty((B, F, C), dtype=torch.int16, device=X.device),
                    torch.empty((B, F, C), dtype=torch.int32, device=X.device))
        return out

    def quantize(self, mdct_amplitudes, masking_threshold):
        """Perceptual quantiser: X, thr [B, F, N, C] float32 -> (codes int16 [B, F, N, C], sf int8 [B, F, M, C]).

        Per scale-factor band (:attr:`scale_band_offsets`) and (clip, frame, channel) a step 2^(sf/4) with
        step * sqrt(3) <= the band's smallest threshold, so the error of a bin is at most thr / (2 sqrt 3), and the noise
        RMS at most the thr / 6 of :meth:`add_noise`; sf = -128 marks a band holding NaN / Inf (its codes are 0).  On a model
        made by :meth:`with_row_budget`: the codes and sf of :meth:`quantize_to_budget` at that budget.  Not
        differentiable (:meth:`add_noise` is the differentiable stand-in); float32 only."""
        X, thr = self._check_quant_inputs(mdct_amplitudes, masking_threshold)
        B, F, N, C = X.shape
        codes, sf = self._alloc_codes(X)
        with _host.on_device(X.device):
            _lib.check(self._lib.ac_quantize(self._plans.get(X.device), _host.ptr(X), _host.ptr(thr), _host.ptr(codes),
                                             _host.ptr(sf), B, F, C, _host.stream_ptr(X.device)))
        return codes, sf

    def _check_codes(self, codes, sf):
        codes = self._check_quant_tensor(codes, "codes", torch.int16)
        B, F, N, C = codes.shape
        if N != self.filter_bands_n:
            raise ValueError("axis 2 of codes (%d) != filter_bands_n (%d)" % (N, self.filter_bands_n))
        sf = self._check_quant_tensor(sf, "sf", torch.int8, (B, F, self.bark_bands_n, C), codes.device)
        return codes, sf

    def dequantize(self, codes, sf):
        """Inverse map of :meth:`quantize`: X^ = fp32(code * 2^(sf/4)) [B, F, N, C] float32 (NaN in bands with sf = -128)."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        codes, sf = self._check_codes(codes, sf)
        B, F, N, C = codes.shape
        X = torch.empty((B, F, N, C), dtype=torch.float32, device=codes.device)
        with _host.on_device(codes.device):
            _lib.check(self._lib.ac_dequantize(self._plans.get(codes.device), _host.ptr(codes), _host.ptr(sf), _host.ptr(X),
                                               B, F, C, _host.stream_ptr(codes.device)))
        return X

    # ---- rate control (extension) ------------------------------------------------
    def quantize_to_budget(self, mdct_amplitudes, masking_threshold, row_bits, min_offset=0):
        """:meth:`quantize` with every scale factor of a (clip, frame, channel) row raised by one offset, the smallest in
        ``[min_offset, 254]`` whose packed row (:meth:`pack`, before its padding to 32 bits) is at most ``row_bits`` long:
        X, thr [B, F, N, C] float32 -> (codes int16 [B, F, N, C], sf int8 [B, F, M, C], offset int16 [B, F, C],
        row_bits_out int32 [B, F, C]).

        ``row_bits`` is an int (at least 5 * bark_bands_n, the length of a row that stores no band) or an int32 tensor
        [B, F, C] of per-row budgets.  A row that cannot meet its budget gets offset 254 and ``row_bits_out`` above it.
        Each unit of offset makes the row's steps 2^(1/4) coarser; scale factors stay in [-127, 127], empty bands keep 0 and
        bands with NaN / Inf keep -128.  ``min_offset`` in [-254, 254]: 0 with an unlimited budget gives :meth:`quantize`,
        a fixed budget of 16N + 13M and a fixed ``min_offset`` is a constant-quality mode.  One launch; not
        differentiable; float32 only."""
        X, thr = self._check_quant_inputs(mdct_amplitudes, masking_threshold)
        B, F, N, C = X.shape
        self._check_min_offset(min_offset)
        scalar, per_row = self._check_row_bits(row_bits, (B, F, C), X.device)
        dev = X.device
        codes, sf, offset, bits = self._alloc_codes(X, rate=True)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_quantize_budget(
                self._plans.get(dev), _host.ptr(X), _host.ptr(thr), scalar, _host.ptr(per_row) if per_row is not None else None,
                int(min_offset), _host.ptr(codes), _host.ptr(sf), _host.ptr(offset), _host.ptr(bits), B, F, C,
                _host.stream_ptr(dev)))
        return codes, sf, offset, bits

    def _check_row_bits(self, row_bits, shape, device):
        """A row budget as the entry points take it: (scalar, None) for an int, (0, int32 tensor of ``shape``) per row."""
        if isinstance(row_bits, torch.Tensor):
            return 0, self._check_quant_tensor(row_bits, "row_bits", torch.int32, shape, device, ndim=3)
        if isinstance(row_bits, (int, np.integer)) and not isinstance(row_bits, bool):
            if not 5 * self.bark_bands_n <= int(row_bits) <= 2 ** 31 - 1:
                raise ValueError("row_bits (%d) below 5 * bark_bands_n = %d, the length of a row that stores no band, or "
                                 "above int32" % (row_bits, 5 * self.bark_bands_n))
            return int(row_bits), None
        raise TypeError("row_bits must be an int or an int32 tensor [B, F, C], got %s" % type(row_bits).__name__)

    # ---- requantiser (extension) --------------------------------------------------
    def requantize_to_budget(self, codes, sf, row_bits, min_offset=0):
        """:meth:`quantize_to_budget` on rows that are already quantised: codes int16 [B, F, N, C], sf int8 [B, F, M, C] ->
        (codes, sf, offset int16 [B, F, C], row_bits_out int32 [B, F, C]) in new tensors.

        The stored scale factors stand where the quantiser's own stood and ``fp32(code * 2^(sf/4))`` where the spectrum
        stood, so no spectrum and no threshold is needed: every scale factor of a row is raised by the smallest offset in
        ``[min_offset, 254]`` at which the packed row is at most ``row_bits`` long, and the codes are quantised again at
        those steps.  A row that fits already keeps offset 0 and comes back as it was (a code of -32768 as -32767).
        ``row_bits`` as in :meth:`quantize_to_budget`; ``min_offset`` in [0, 254] -- an offset below 0 cannot restore
        what the first quantiser dropped.  The input need not be canonical: codes under ``sf = -128`` count as 0 and an
        all-zero band as ``sf = 0``, as :meth:`unpack` returns them.  One launch; not differentiable; float32 only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        self._check_min_offset(min_offset)
        if int(min_offset) < 0:
            raise ValueError("min_offset (%d) outside [0, 254]: requantising cannot lower a scale factor" % min_offset)
        codes, sf = self._check_codes(codes, sf)
        B, F, N, C = codes.shape
        scalar, per_row = self._check_row_bits(row_bits, (B, F, C), codes.device)
        dev = codes.device
        out_codes, out_sf, offset, bits = self._alloc_codes(codes, rate=True)
        rows = _lib.QuantizedRows(codes.data_ptr(), sf.data_ptr())
        if codes.numel() == 0:
            return out_codes, out_sf, offset, bits
        with _host.on_device(dev):
            _lib.check(self._lib.ac_quantize_budget(
                self._plans.get(dev), ctypes.addressof(rows), None, scalar, _host.ptr(per_row) if per_row is not None else None,
                int(min_offset), _host.ptr(out_codes), _host.ptr(out_sf), _host.ptr(offset), _host.ptr(bits), B, F, C,
                _host.stream_ptr(dev)))
        return out_codes, out_sf, offset, bits

    # ---- mixing quantised rows (extension) ----------------------------------------
    @staticmethod
    def _check_gains(gains, sources_n):
        """``gains`` of a mix as a list of ``sources_n`` ints in [-254, 254]; None: zeros."""
        if gains is None:
            return [0] * sources_n
        gains = list(gains)
        if len(gains) != sources_n:
            raise ValueError("%d gains for %d sources" % (len(gains), sources_n))
        for g in gains:
            if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
                raise TypeError("a gain must be an int (scale-factor units of 2^(1/4)), got %s" % type(g).__name__)
            if not -254 <= int(g) <= 254:
                raise ValueError("gain (%d) outside [-254, 254]" % g)
        return [int(g) for g in gains]

    def _check_active(self, active, sources_n, shape, device):
        """``active`` of a mix: None, or a uint8 / bool tensor [S, B, F, C] on ``device``; returned as uint8."""
        if active is None:
            return None
        if not isinstance(active, torch.Tensor):
            raise TypeError("active must be a torch.Tensor or None, got %s" % type(active).__name__)
        if active.dtype not in (torch.uint8, torch.bool):
            raise ValueError("active has dtype %s, expected torch.uint8 or torch.bool" % active.dtype)
        if tuple(active.shape) != (sources_n,) + tuple(shape):
            raise ValueError("active must have shape %s, got %s" % ((sources_n,) + tuple(shape), tuple(active.shape)))
        if active.device != device:
            raise ValueError("active lives on %s but the rows on %s" % (active.device, device))
        active = active.contiguous()
        return active.view(torch.uint8) if active.dtype == torch.bool else active

    def _band_of_bins(self, device):
        """int64 [N] on ``device``: the scale-factor band of every bin.  Built on the device from the host's offsets (no
        copy that would wait for it) and kept per device."""
        cache = self._band_ids
        if device not in cache:
            i = torch.arange(self.filter_bands_n, dtype=torch.int64, device=device)
            band = torch.zeros_like(i)
            for o in self.scale_band_offsets[1:-1].tolist():
                band += i >= o
            cache[device] = band
        return cache[device]

    def mix_to_budget(self, rows, gains, row_bits, active=None):
        """Sums quantised rows of several sources in the spectral domain and quantises the sum to a budget (DESIGN.md
        section 8h): ``rows`` a list of S pairs (codes int16 [B, F, N, C], sf int8 [B, F, M, C]) of equal shapes on one
        device -> (codes, sf, offset int16 [B, F, C], row_bits_out int32 [B, F, C]) as :meth:`quantize_to_budget` returns them.

        ``gains``: S ints in [-254, 254] in scale-factor units (one is 2^(1/4), 1.505 dB), or None; ``active``: None or a
        uint8 / bool tensor [S, B, F, C], 0 = the row adds nothing.  Source i is dequantised at ``clamp(sf + gains[i], -127,
        127)`` (a band with sf = -128 stays one: NaN), the spectra are added in float32 in source order, and the sum is
        quantised by :meth:`quantize_to_budget` from offset 0 under a threshold that makes its scale factor at offset 0 the
        band's s0: -128 where a source has the band at -128, else the largest gained scale factor over the sources that hold
        a non-zero code in it, else 0 -- the coarsest step wins.  The input need not be canonical (as in
        :meth:`requantize_to_budget`).  2 S + 1 library launches between torch's own; nothing waits for the device.
        ``row_bits`` as in :meth:`quantize_to_budget`; not differentiable; float32 only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        rows = list(rows)
        if not rows:
            raise ValueError("mix_to_budget needs at least one source")
        gains = self._check_gains(gains, len(rows))
        pairs = []
        for i, pair in enumerate(rows):
            codes, sf = self._check_codes(*pair)
            if pairs and (codes.shape != pairs[0][0].shape or codes.device != pairs[0][0].device):
                raise ValueError("source %d has codes of shape %s on %s, source 0 of shape %s on %s"
                                 % (i, tuple(codes.shape), codes.device, tuple(pairs[0][0].shape), pairs[0][0].device))
            pairs.append((codes, sf))
        B, F, N, C = pairs[0][0].shape
        M, dev = self.bark_bands_n, pairs[0][0].device
        active = self._check_active(active, len(pairs), (B, F, C), dev)
        band = self._band_of_bins(dev)
        total = bad = s0 = None
        for i, (codes, sf) in enumerate(pairs):
            is_bad = sf == -128
            g = torch.where(is_bad, -128, (sf.to(torch.int16) + gains[i]).clamp_(-127, 127)).to(torch.int16)
            X = self.dequantize(codes, g.to(torch.int8))
            holds = torch.zeros((B, F, M, C), dtype=torch.int32, device=dev).index_add_(2, band, (codes != 0).to(torch.int32)) > 0
            stored = holds & ~is_bad
            if active is not None:
                on = active[i].unsqueeze(2) != 0
                X = torch.where(on, X, 0.0)
                is_bad, stored = is_bad & on, stored & on
            cand = torch.where(stored, g, -129)
            total = X if total is None else total + X
            bad = is_bad if bad is None else bad | is_bad
            s0 = cand if s0 is None else torch.maximum(s0, cand)
        s = torch.where(bad | (s0 == -129), 0, s0).to(torch.int32)   # (any finite threshold does where the band is bad)
        r = s & 3
        mant = torch.where(r == 0, 0, torch.where(r == 1, 0x1837f0, torch.where(r == 2, 0x3504f3, 0x5744fd))).to(torch.int32)
        step = (((127 + (s >> 2)) << 23) | mant).view(torch.float32)      # step(s) = ldexp(fp32(2^((s & 3) / 4)), s >> 2)
        thr = (step * float(np.float32(np.sqrt(np.float32(3.0))))).index_select(2, band)
        return self.quantize_to_budget(total, thr, row_bits, 0)

    # ---- the level of quantised rows (extension) -----------------------------------
    def level(self, codes, sf):
        """The energy of quantised rows from their codes and scale factors: codes int16 [B, F, N, C],
        sf int8 [B, F, M, C] -> (energy float32 [B, F, C], bad uint8 [B, F, C]).

        Per band j: Q_j, the sum of the squared codes as an exact integer, times w(sf_j) = fp32(step step) of the band's
        step, one float32 product; a band with sf = -128 is *bad* and adds +0.  The 64 (or next power of two) band energies
        are added as the fold tree ``v[i] += v[i + d]``, d = P/2 ... 1, so the value equals, bit for bit, what a wave's xor
        butterfly gives.  ``energy`` is the sum of :meth:`dequantize` squared over the row's good bands within 2^-20
        relative, finite and never negative; ``bad`` is 1 where any band of the row is bad.  Any filter_bands_n and band
        layout; torch operations only, nothing waits for the device.  float32 plans only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        codes, sf = self._check_codes(codes, sf)
        B, F, N, C = codes.shape
        M, dev = self.bark_bands_n, codes.device
        band = self._band_of_bins(dev)
        is_bad = sf == -128
        q = codes.to(torch.int64)
        Q = torch.zeros((B, F, M, C), dtype=torch.int64, device=dev).index_add_(2, band, q * q)   # (integer adds: exact)
        s = torch.arange(-127, 128, dtype=torch.int32, device=dev)
        r = s & 3
        mant = torch.where(r == 0, 0, torch.where(r == 1, 0x1837f0, torch.where(r == 2, 0x3504f3, 0x5744fd))).to(torch.int32)
        step = (((127 + (s >> 2)) << 23) | mant).view(torch.float32)      # step(s) = ldexp(fp32(2^((s & 3) / 4)), s >> 2)
        w = (step * step)[(sf.to(torch.int64) + 127).clamp_(min=0)]       # the 255-entry table, looked up per band
        e = torch.where(is_bad, 0.0, Q.to(torch.float32) * w)
        P = 1
        while P < M:
            P *= 2
        v = torch.zeros((B, F, C, P), dtype=torch.float32, device=dev)
        v[..., :M] = e.permute(0, 1, 3, 2)
        while P > 1:
            P //= 2
            v = v[..., :P] + v[..., P:2 * P]
        return v[..., 0].contiguous(), is_bad.any(dim=2).to(torch.uint8)

    # ---- rate control per clip (extension) ---------------------------------------
    def quantize_to_clip_budget(self, mdct_amplitudes, masking_threshold, clip_bits, min_offset=0):
        """:meth:`quantize_to_budget` with one budget for the whole clip: X, thr [B, F, N, C] float32 -> (codes int16
        [B, F, N, C], sf int8 [B, F, M, C], offset int16 [B, F, C], row_bits_out int32 [B, F, C], clip_bits_out int64 [B]).

        ``clip_bits`` is an int (at least F * C * 32 * ceil(5 * bark_bands_n / 32), the length of a clip that stores no
        band) or an int64 tensor [B] of per-clip budgets.  A clip's rows, padded to 32 bits as :meth:`pack` stores them,
        take the smallest offset k in ``[min_offset, 254]`` at which their total is at most the budget; the bits left
        over then lower the first rows of the clip (frame by frame, channel by channel) to k - 1 as far as they reach.
        ``clip_bits_out`` is the clip's length in ``pack()``'s data in bits; a clip that cannot meet its budget gets
        offset 254 and ``clip_bits_out`` above it.  No host synchronisation; not differentiable; float32 only."""
        X, thr = self._check_quant_inputs(mdct_amplitudes, masking_threshold)
        B, F, N, C = X.shape
        self._check_min_offset(min_offset)
        per_clip = None
        scalar = 0
        if isinstance(clip_bits, torch.Tensor):
            per_clip = self._check_quant_tensor(clip_bits, "clip_bits", torch.int64, (B,), X.device, ndim=1)
        elif isinstance(clip_bits, (int, np.integer)) and not isinstance(clip_bits, bool):
            floor = F * C * 32 * ((5 * self.bark_bands_n + 31) // 32)
            if not floor <= int(clip_bits) <= 2 ** 63 - 1:
                raise ValueError("clip_bits (%d) below frames * channels * 32 * ceil(5 * bark_bands_n / 32) = %d, the length "
                                 "of a clip that stores no band, or above int64" % (clip_bits, floor))
            scalar = int(clip_bits)
        else:
            raise TypeError("clip_bits must be an int or an int64 tensor [B], got %s" % type(clip_bits).__name__)
        dev = X.device
        codes, sf, offset, bits = self._alloc_codes(X, rate=True)
        clip_out = torch.empty((B,), dtype=torch.int64, device=dev)
        plan = self._plans.get(dev)
        nscratch = int(self._lib.ac_clip_budget_scratch_bytes(plan, B, F, C))
        scratch = torch.empty((nscratch,), dtype=torch.uint8, device=dev) if nscratch else None
        with _host.on_device(dev):
            _lib.check(self._lib.ac_quantize_clip_budget(
                plan, _host.ptr(X), _host.ptr(thr), scalar, _host.ptr(per_clip) if per_clip is not None else None,
                int(min_offset), _host.ptr(codes), _host.ptr(sf), _host.ptr(offset), _host.ptr(bits), None,
                _host.ptr(clip_out), _host.ptr(scratch) if scratch is not None else None, B, F, C, _host.stream_ptr(dev)))
        return codes, sf, offset, bits, clip_out

    # ---- packed bitstream of quantised spectra (extension) ------------------------
    def pack(self, codes, sf):
        """Packs :meth:`quantize` output into a bitstream: codes int16 [B, F, N, C], sf int8 [B, F, M, C] ->
        (data uint8 [nbytes], index int64 [B, F, C]).

        Every (clip, frame, channel) row stores each scale-factor band at the bit width its largest zigzag code needs
        (DESIGN.md section 8b has the format); ``index`` holds each row's byte offset in ``data``.  Any int16 code and
        int8 sf is accepted.  Three launches around one device-to-host read of the byte count: the call synchronises
        with the device and cannot be captured in a graph.  float32 plans only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        codes, sf = self._check_codes(codes, sf)
        B, F, N, C = codes.shape
        dev = codes.device
        index = torch.empty((B, F, C), dtype=torch.int64, device=dev)
        total = torch.empty((1,), dtype=torch.int64, device=dev)
        nscratch = int(self._lib.ac_pack_scratch_bytes(B, F, C))
        scratch = torch.empty((nscratch,), dtype=torch.uint8, device=dev) if nscratch else None
        plan = self._plans.get(dev)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_pack_index(plan, _host.ptr(codes), _host.ptr(sf), _host.ptr(index), _host.ptr(total),
                                               _host.ptr(scratch) if scratch is not None else None, B, F, C,
                                               _host.stream_ptr(dev)))
            data = torch.empty((int(total.item()),), dtype=torch.uint8, device=dev)
            _lib.check(self._lib.ac_pack(plan, _host.ptr(codes), _host.ptr(sf), _host.ptr(index), _host.ptr(data), B, F, C,
                                         _host.stream_ptr(dev)))
        return data, index

    def unpack(self, data, index):
        """Inverse of :meth:`pack`: data uint8 [nbytes], index int64 [B', F', C] -> (codes int16 [B', F', N, C],
        sf int8 [B', F', M, C]) in canonical form -- codes 0 in bands with sf = -128, sf 0 in bands whose codes are all 0
        (:meth:`dequantize` gives the same values as on the packed input).  ``index`` may hold any row starts, e.g. a
        slice of frames or channels in another order.  Bits past the end of ``data`` read as 0.  float32 plans only."""
        _host.require_float32(self.compute_dtype, "the quantiser")
        data = self._check_quant_tensor(data, "data", torch.uint8, ndim=1)
        index = self._check_quant_tensor(index, "index", torch.int64, device=data.device, ndim=3)
        B, F, C = index.shape
        dev = data.device
        codes = torch.empty((B, F, self.filter_bands_n, C), dtype=torch.int16, device=dev)
        sf = torch.empty((B, F, self.bark_bands_n, C), dtype=torch.int8, device=dev)
        with _host.on_device(dev):
            _lib.check(self._lib.ac_unpack(self._plans.get(dev), _host.ptr(data), data.numel(), _host.ptr(index),
                                           _host.ptr(codes), _host.ptr(sf), B, F, C, _host.stream_ptr(dev)))
        return codes, sf

    # ---- concealment of lost rows (extension) -------------------------------------
    @staticmethod
    def _check_max_age(max_age):
        if isinstance(max_age, bool) or not isinstance(max_age, (int, np.integer)):
            raise TypeError("max_age must be an int, got %s" % type(max_age).__name__)
        if not 0 <= int(max_age) <= _lib.AC_CONCEAL_MAX_AGE:
            raise ValueError("max_age (%d) outside [0, %d]" % (max_age, _lib.AC_CONCEAL_MAX_AGE))
        return int(max_age)

    def _check_lost(self, lost, index):
        """``lost`` uint8 / bool with ``index``'s shape and device -> uint8, ready for the kernels."""
        if not isinstance(lost, torch.Tensor):
            raise TypeError("lost must be a torch.Tensor, got %s" % type(lost).__name__)
        if lost.dtype not in (torch.uint8, torch.bool):
            raise ValueError("lost has dtype %s, expected torch.uint8 or torch.bool" % lost.dtype)
        lost = self._check_quant_tensor(lost, "lost", lost.dtype, index.shape, index.device, ndim=3)
        return lost.view(torch.uint8)

    @staticmethod
    def _check_redundant_at(redundant_at):
        if isinstance(redundant_at, bool) or not isinstance(redundant_at, (int, np.integer)):
            raise TypeError("redundant_at must be an int, got %s" % type(redundant_at).__name__)
        if not 1 <= int(redundant_at) < 2 ** 31:
            raise ValueError("redundant_at (%d) outside [1, 2^31)" % redundant_at)
        return int(redundant_at)

    def conceal_plan(self, index, lost, nbytes, max_age=8, redundant_at=None):
        """Where each row of a stream with lost rows is read from: index int64 [B, F, C], lost uint8 / bool [B, F, C]
        (nonzero: the row did not arrive) -> (src_index int64 [B, F, C], age uint8 [B, F, C]).

        ``age`` is the smallest a in [0, min(max_age, f)] with ``lost[b, f-a, c] == 0`` and ``src_index`` is
        ``index[b, f-a, c]``: the last row of the same clip and channel that arrived.  Where there is none -- a run of
        lost rows longer than ``max_age``, or lost rows before the first good one -- the row is muted: ``src_index`` is
        ``nbytes``, a row :meth:`unpack` reads as silence, and ``age`` 0.  Torch ops on the current stream.

        ``redundant_at`` (an int in [1, 2^31)): ahead of that rule, a lost row whose successor
        arrived -- ``f + 1 < F`` and ``lost[b, f+1, c] == 0`` -- is recovered: ``src_index`` is
        ``index[b, f+1, c] + redundant_at``, the copy the successor's slot carries, and ``age`` 0."""
        max_age = self._check_max_age(max_age)
        if redundant_at is not None:
            redundant_at = self._check_redundant_at(redundant_at)
        index = self._check_quant_tensor(index, "index", torch.int64, ndim=3)
        lost = self._check_lost(lost, index)
        B, F, C = index.shape
        if F == 0:
            return index.clone(), torch.zeros((B, F, C), dtype=torch.uint8, device=index.device)
        f = torch.arange(F, dtype=torch.int64, device=index.device).view(1, F, 1)
        last = f.expand(B, F, C).masked_fill(lost != 0, -1).cummax(dim=1).values   # the last frame <= f that arrived
        found = (last >= 0) & (f - last <= max_age)
        src_index = index.gather(1, last.clamp(min=0)).masked_fill(~found, int(nbytes))
        age = (f - last).masked_fill(~found, 0).to(torch.uint8)
        if redundant_at is not None and F >= 2:
            recovered = (lost[:, :-1] != 0) & (lost[:, 1:] == 0)
            src_index[:, :-1] = torch.where(recovered, index[:, 1:] + redundant_at, src_index[:, :-1])
            age[:, :-1].masked_fill_(recovered, 0)
        return src_index, age

    def conceal_fade(self, sf, age):
        """The scale factors of concealed rows: sf int8 [B, F, M, C], age uint8 [B, F, C] -> every ``s != -128`` replaced
        by ``max(s - AC_CONCEAL_FADE * age, -127)``: the spectrum times ``2^-age``.  ``-128`` stays."""
        sf = self._check_quant_tensor(sf, "sf", torch.int8)
        B, F, _, C = sf.shape
        age = self._check_quant_tensor(age, "age", torch.uint8, (B, F, C), sf.device, ndim=3)
        low = (sf.to(torch.int16) - _lib.AC_CONCEAL_FADE * age.to(torch.int16).unsqueeze(2)).clamp(min=-127).to(torch.int8)
        return torch.where(sf == -128, sf, low)

    # ---- Bark scale (host precompute helpers, psychoacoustic.py:333-339) ------------------------------
    def freq2bark(self, frequencies):
        """Empirical Bark scale (``:333-335``)."""
        return 6.0 * torch.asinh(torch.as_tensor(frequencies, dtype=torch.float64) / 600.0)

    def bark2freq(self, bark_band):
        """Empirical Bark scale (``:337-339``)."""
        return 600.0 * torch.sinh(torch.as_tensor(bark_band, dtype=torch.float64) / 6.0)
