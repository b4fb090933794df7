"""The float64 torch restatement of the filter bank (tests/mdct_torch_reference.py) against the float64 oracle, on the host:
the reference gradients of tests/test_mdct_backward.py are torch.autograd on this restatement, so its forward and inverse
must be the oracle's, and its gradients the transposes of the oracle's linear maps.  No GPU needed."""

import numpy as np
import pytest
import torch

import mdct_torch_reference as ref

from oracle.audiocodec_oracle import MDCTOracle

WINDOWS = ["vorbis", "sine", "rect", None]
SIZES = [16, 30, 34, 64, 96, 960, 1024, 8190, 8192]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("pre", ["float64", "float32"])
@pytest.mark.parametrize("wt", WINDOWS)
@pytest.mark.parametrize("N", SIZES)
def test_restatement_equals_the_oracle(N, wt, pre, C):
    K, B = (2, 1) if N > 1024 else (3, 2)
    pdt = np.float32 if pre == "float32" else np.float64
    o = MDCTOracle(N, wt, np.float64, precompute_dtype=pdt)
    coef = ref.fold_coef(N, wt, pdt)
    g = np.random.default_rng(N + C)
    x = g.uniform(-1, 1, (B, K * N, C))
    Xo = o.transform(x)
    assert _rel(ref.transform(torch.from_numpy(x), coef).numpy(), Xo) <= 1e-12
    Xv = g.standard_normal((B, K, N, C))
    assert _rel(ref.inverse_transform(torch.from_numpy(Xv), coef).numpy(), o.inverse_transform(Xv)) <= 1e-12


@pytest.mark.parametrize("N,wt,pre,C", [(16, "rect", "float64", 3), (30, "vorbis", "float64", 1), (34, "sine", "float32", 2),
                                         (64, "vorbis", "float32", 2), (96, None, "float64", 1), (96, "sine", "float64", 3)])
def test_restatement_gradients_equal_the_dense_maps(N, wt, pre, C):
    """T^T g and S^T g by autograd on the restatement equal the oracle's linear maps, assembled column by column from
    oracle.transform / inverse_transform on unit impulses (as test_gpu_parity.py's autograd tests build them)."""
    K, B = 3, 2
    pdt = np.float32 if pre == "float32" else np.float64
    o = MDCTOracle(N, wt, np.float64, precompute_dtype=pdt)
    coef = ref.fold_coef(N, wt, pdt)
    g = np.random.default_rng(N)
    x = torch.from_numpy(g.uniform(-1, 1, (B, K * N, C)))
    gX = torch.from_numpy(g.standard_normal((B, K + 1, N, C)))
    T = o.transform(np.eye(K * N).reshape(K * N, K * N, 1)).reshape(K * N, (K + 1) * N)      # row i = T e_i
    gx_ref = np.einsum("if,bfc->bic", T, gX.numpy().reshape(B, (K + 1) * N, C))
    assert _rel(ref.transform_grad(x, gX, coef).numpy(), gx_ref) <= 1e-12
    Xv = torch.from_numpy(g.standard_normal((B, K, N, C)))
    gy = torch.from_numpy(g.standard_normal((B, (K + 1) * N, C)))
    S = o.inverse_transform(np.eye(K * N).reshape(K * N, K, N, 1)).reshape(K * N, (K + 1) * N)   # row i = S e_i
    gX_ref = np.einsum("is,bsc->bic", S, gy.numpy()).reshape(B, K, N, C)
    assert _rel(ref.inverse_grad(Xv, gy, coef).numpy(), gX_ref) <= 1e-12


@pytest.mark.parametrize("N", [16, 96, 1024])
def test_restatement_does_not_take_the_orthogonal_fold_shortcut(N):
    """For the rectangular window the fold blocks [[1, 1], [1, 0]] are not rotations: T^T g from autograd differs from
    inverse_transform(g) / 4N by far more than rounding, while for a Princen-Bradley window the two agree (to the float64
    rounding of the fold constants: the lower-right entry cancels where the window is small)."""
    K, B, C = 3, 1, 2
    g = torch.from_numpy(np.random.default_rng(N).standard_normal((B, K + 1, N, C)))
    x = torch.zeros(B, K * N, C, dtype=torch.float64)
    for wt, same in (("rect", False), ("vorbis", True)):
        coef = ref.fold_coef(N, wt)
        gx = ref.transform_grad(x, g, coef)
        shortcut = ref.inverse_transform(g, coef)[:, N:-N] / (4.0 * N)
        assert (_rel(shortcut.numpy(), gx.numpy()) <= 1e-9) == same
        if not same:
            assert _rel(shortcut.numpy(), gx.numpy()) > 0.1
