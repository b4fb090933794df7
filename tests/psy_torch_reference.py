"""The masking model restated in float64 torch ops (test infrastructure: lets torch.autograd produce reference gradients
for the adjoint kernels of tonality / global_masking_threshold).  The constants come from a ``PsychoacousticModel`` (built
on the host, no device needed); everything runs on the device of ``X``."""

import numpy as np
import torch


def torch_masking_intensity(p, X, t, drown, S=None):
    """``_masking_intensity_in_bark`` (psychoacoustic.py:169-210): the masking intensity T [B,F,M,C] before the maximum
    with the quiet threshold, float64.  ``S`` replaces the model's spreading matrix (the tests' sensitivity guards)."""
    d = X.device
    W = p.W.double().to(d)
    S = (p.spreading_matrix if S is None else S).double().to(d)
    alpha, M = float(p.alpha), p.bark_bands_n
    eps = 1e-14
    I = X ** 2
    P = torch.einsum("nbic,ij->nbjc", I, W)
    Q = torch.clamp(P, min=eps) ** alpha
    A = torch.einsum("nbic,ij->nbjc", Q, S)
    # (the reference evaluates linspace in compute_dtype, psychoacoustic.py:187-189: float32 unless the model is float64)
    bdt = torch.float64 if p.compute_dtype == torch.float64 else torch.float32
    beta = torch.linspace(0.0, float(p.max_bark), M, dtype=bdt).double().to(d).reshape(1, 1, M, 1)
    O = (1.0 - drown) * (t * beta + 9.0 * t + 5.5)
    fac = 10.0 ** (-alpha * O / 10.0)
    return torch.clamp(fac * A, min=eps) ** (1.0 / alpha)


def torch_psy_reference(p, X, t, drown, S=None):
    """``global_masking_threshold`` (psychoacoustic.py:122-148 with 169-210, 301-331) of the model ``p`` at X [B,F,N,C] and
    t [B,F,1,C], float64."""
    d = X.device
    Wi = p.W_inv.double().to(d)
    quiet = p.quiet_threshold_intensity.double().to(d)
    eps = 1e-14
    G = torch.maximum(torch_masking_intensity(p, X, t, drown, S), quiet)
    E = torch.einsum("nbjc,jf->nbfc", G, Wi)
    return torch.sqrt(torch.clamp(E, min=eps))


def torch_tonality_reference(X):
    """``tonality`` (psychoacoustic.py:102-120) of X [B,F,N,C] -> [B,F,1,C], float64."""
    eps = 1e-14
    I = X ** 2
    sfm = 10.0 * (torch.log(torch.clamp(I, min=eps)).mean(dim=2, keepdim=True)
                  - torch.log(I.mean(dim=2, keepdim=True) + eps)) / np.log(10.0)
    return torch.clamp(sfm / -60.0, max=1.0)


def oracle_constants(o):
    """The constants of a ``PsychoOracle`` in the attribute names ``torch_psy_reference`` reads (float64 tensors)."""
    from types import SimpleNamespace
    return SimpleNamespace(W=torch.from_numpy(o.W64), W_inv=torch.from_numpy(o.W_inv64),
                           spreading_matrix=torch.from_numpy(o.spreading64),
                           quiet_threshold_intensity=torch.from_numpy(o.quiet64), alpha=o.alpha,
                           bark_bands_n=o.bark_bands_n, max_bark=float(o.max_bark), compute_dtype=torch.float64)
