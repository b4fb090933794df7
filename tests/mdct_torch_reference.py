"""The filter bank restated in float64 torch ops (test infrastructure: lets torch.autograd produce reference gradients for
the transposed bank that runs the backward of transform / inverse_transform).  It follows the oracle's ``MDCTOracle``
(oracle/audiocodec_oracle.py) step by step, the scales 1/sqrt(4N) and sqrt(4N) included, and takes the fold coefficients
from ``oracle.fold_coefficients``.  The DCT-IV is a 2N-point complex FFT, so any even N serves (up to 8192 and beyond) on
the host or the device of the input, without a dense N x N matrix."""

import math

import numpy as np
import torch

from oracle.audiocodec_oracle import fold_coefficients


def fold_coef(N, window_type, precompute_dtype=np.float64, device="cpu"):
    """The eight fold vectors (a1..a4, s1..s4) of ``oracle.fold_coefficients`` as float64 tensors on ``device``."""
    c = fold_coefficients(N, window_type, precompute_dtype)
    return {k: torch.from_numpy(np.asarray(c[k], dtype=np.float64)).to(device) for k in
            ("a1", "a2", "a3", "a4", "s1", "s2", "s3", "s4")}


def dct4(v):
    """Orthonormal DCT-IV on the last axis (``MDCTOracle._dct4``): y[k] = sqrt(2/N) sum_n v[n] cos(pi/N (n+1/2)(k+1/2)),
    as Re(exp(-i pi (k+1/2) / 2N) FFT_2N(v[n] exp(-i pi n / 2N))[k])."""
    N = v.shape[-1]
    n = torch.arange(N, dtype=torch.float64, device=v.device)
    pre = torch.exp(torch.complex(torch.zeros_like(n), -math.pi * n / (2 * N)))
    post = torch.exp(torch.complex(torch.zeros_like(n), -math.pi * (n + 0.5) / (2 * N)))
    y = torch.fft.fft(v.to(torch.complex128) * pre, n=2 * N, dim=-1)[..., :N]
    return math.sqrt(2.0 / N) * (y * post).real


def transform(x, coef):
    """``MDCTOracle.transform``: x [B, K*N, C] -> X [B, K+1, N, C], float64."""
    B, S, C = x.shape
    N = coef["a1"].shape[0] * 2
    h = N // 2
    K = S // N
    xb = x.permute(0, 2, 1).reshape(B * C, K, N)
    zero = torch.zeros(B * C, 1, N, dtype=x.dtype, device=x.device)
    cur = torch.cat([xb, zero], dim=1)                                   # block n     (x_K  = 0)
    prv = torch.cat([zero, xb], dim=1)                                   # block n-1   (x_-1 = 0)
    hi = coef["a1"] * cur[..., :h] + coef["a2"] * cur[..., h:].flip(-1)      # v[h+j]
    lo = coef["a3"] * prv[..., :h].flip(-1) + coef["a4"] * prv[..., h:]      # v[j]
    y = dct4(torch.cat([lo, hi], dim=-1))
    return y.reshape(B, C, K + 1, N).permute(0, 2, 3, 1) / math.sqrt(4.0 * N)


def inverse_transform(X, coef):
    """``MDCTOracle.inverse_transform``: X [B, K', N, C] -> x [B, (K'+1)*N, C], float64."""
    B, Kp, N, C = X.shape
    h = N // 2
    u = dct4(math.sqrt(4.0 * N) * X.permute(0, 3, 1, 2).reshape(B * C, Kp, N))
    zero = torch.zeros(B * C, 1, N, dtype=X.dtype, device=X.device)
    a = torch.cat([u, zero], dim=1)[..., :h].flip(-1)                    # u_n[h-1-j]      (u_K' = 0)
    b = torch.cat([zero, u], dim=1)[..., h:]                             # u_{n-1}[h+j]    (u_-1 = 0)
    lo = coef["s1"] * a + coef["s2"] * b                                 # out[j]
    hi = (coef["s3"] * a + coef["s4"] * b).flip(-1)                      # out[N-1-j]
    out = torch.cat([lo, hi], dim=-1)
    return out.reshape(B, C, (Kp + 1) * N).permute(0, 2, 1)


def transform_grad(x, g, coef):
    """T^T g: the gradient of sum(transform(x) * g) w.r.t. x, by torch.autograd on the restatement."""
    xd = x.detach().double().requires_grad_(True)
    (transform(xd, coef) * g.detach().double()).sum().backward()
    return xd.grad


def inverse_grad(X, g, coef):
    """S^T g: the gradient of sum(inverse_transform(X) * g) w.r.t. X, by torch.autograd on the restatement."""
    Xd = X.detach().double().requires_grad_(True)
    (inverse_transform(Xd, coef) * g.detach().double()).sum().backward()
    return Xd.grad
