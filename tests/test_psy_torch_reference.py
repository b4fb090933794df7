"""The float64 torch restatement of the masking model (tests/psy_torch_reference.py) against the float64 oracle, on the
host: the reference gradients of tests/test_psy_backward.py are torch.autograd on this restatement, so its forward must
be the oracle's.  No GPU needed."""

import numpy as np
import pytest
import torch

from psy_torch_reference import oracle_constants, torch_psy_reference, torch_tonality_reference

from oracle.audiocodec_oracle import PsychoOracle

# the layouts of tests/test_psy_backward.py: the wave-level sizes, general layouts, and more than 64 bands
LAYOUTS = [(48000, 1024, 64, 1), (44100, 2048, 64, 3), (48000, 30, 8, 1), (32768, 64, 64, 3), (48000, 120, 20, 7),
           (48000, 960, 64, 3), (48000, 4096, 64, 2), (48000, 1024, 100, 1), (48000, 1024, 128, 3), (48000, 512, 200, 2),
           (48000, 2048, 256, 1)]


@pytest.mark.parametrize("sr,N,M,C", LAYOUTS)
def test_restatement_forward_equals_the_oracle(sr, N, M, C):
    g = torch.Generator().manual_seed(N + M + C)
    env = torch.logspace(-4, 0, N, dtype=torch.float64).reshape(1, 1, N, 1)
    X = (torch.rand(2, 3, N, C, generator=g, dtype=torch.float64) * 2 - 1) * env
    X[0, 0, :, 0] = 0.0                                     # a silent frame: every clamp at eps
    X[1, 1, :, -1] = 1e-6 * (1 + torch.rand(N, generator=g, dtype=torch.float64))
    X[1, 1, N // 3, -1] = 0.9                               # one tone over a floor: tonality clamped at 1
    o = PsychoOracle(sr, N, M, compute_dtype=np.float64)
    c = oracle_constants(o)
    to = o.tonality(X.numpy())
    t = torch_tonality_reference(X)
    assert float(t[1, 1, 0, -1]) == 1.0 and to[1, 1, 0, -1] == 1.0
    assert np.max(np.abs(t.numpy() - to)) <= 1e-12 * max(1.0, np.max(np.abs(to)))
    for drown in (0.0, 0.4, 1.0):
        thr = torch_psy_reference(c, X, t, drown).numpy()
        ref = o.global_masking_threshold(X.numpy(), to, drown)
        assert np.max(np.abs(thr - ref) / ref) <= 1e-12
    # the restatement does see drown: a changed offset is visible far above that bar
    assert np.max(np.abs(torch_psy_reference(c, X, t, 0.45).numpy() - o.global_masking_threshold(X.numpy(), to, 0.4))
                  / o.global_masking_threshold(X.numpy(), to, 0.4)) > 1e-3
