"""CPU: the numpy restatement of the noise generator (tests/noise_reference.py) is itself a standard normal stream.

test_value_contracts.py holds the kernels to the restatement element by element; this module holds the restatement to what
it claims to draw, so that a generator both sides got wrong in the same way (a short period, correlated seeds, a lopsided
Box-Muller) does not pass.  n = 2^20 draws per seed; every bar is 4 sampling standard deviations of the statistic under
the hypothesis (mean 1 / sqrt(n), variance sqrt(2 / n), third moment sqrt(15 / n), fourth sqrt(96 / n), a correlation
1 / sqrt(n)), and the Kolmogorov-Smirnov statistic sqrt(n) D <= 1.95 (0.1 % level).  Measured: moments within 1.5
deviations, lags within 2.3, sqrt(n) D <= 0.83, seeds 7 / 8 correlated 0.26 deviations.
"""

import math

import numpy as np
import pytest

import noise_reference as nr

N_DRAWS = 1 << 20
SEEDS = (0, 5, 2 ** 64 - 1, 1234567)


def _draws(seed, cache={}):
    if seed not in cache:
        g = nr.normals(seed, N_DRAWS)
        g.setflags(write=False)
        cache[seed] = g
    return cache[seed]


def test_mix64_is_splitmix64():
    """The first outputs of splitmix64 from state 0 (the published test vector of the generator)."""
    assert int(nr.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(nr.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert int(nr.mix64(np.uint64(2 ** 64 - 1))) == int(nr.mix64(np.array([2 ** 64 - 1], dtype=np.uint64))[0])


def test_uniforms_and_element_mapping():
    u1, u2 = nr.uniforms(5, np.arange(1 << 16, dtype=np.uint64))
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.all(u1 * 16777216.0 == np.rint(u1 * 16777216.0)) and np.all(u2 * 16777216.0 == np.rint(u2 * 16777216.0))
    c, s = nr.normal_pair(5, np.arange(8, dtype=np.uint64))
    g = nr.normals(5, 16)
    assert np.array_equal(g[0::2], c) and np.array_equal(g[1::2], s)          # element 2p: cos, 2p + 1: sin
    assert np.array_equal(nr.normals(5, 9, first=3), g[3:12])                  # any window of the same stream
    assert np.array_equal(nr.normals(-1, 64), nr.normals(2 ** 64 - 1, 64))     # the seed modulo 2^64
    assert not np.array_equal(nr.normals(0, 64), nr.normals(1, 64))


@pytest.mark.parametrize("seed", SEEDS)
def test_moments(seed):
    g = _draws(seed)
    n = float(g.size)
    assert abs(g.mean()) <= 4.0 / math.sqrt(n)
    assert abs((g ** 2).mean() - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    assert abs((g ** 3).mean()) <= 4.0 * math.sqrt(15.0 / n)
    assert abs((g ** 4).mean() - 3.0) <= 4.0 * math.sqrt(96.0 / n)


@pytest.mark.parametrize("seed", SEEDS)
def test_autocorrelation(seed):
    g = _draws(seed)
    bar = 4.0 / math.sqrt(g.size)
    for lag in (1, 2, 3, 4, 1024, 2048):
        assert abs(float(np.mean(g[:-lag] * g[lag:]))) <= bar, lag


def test_neighbouring_seeds_are_uncorrelated():
    a, b = nr.normals(7, N_DRAWS), nr.normals(8, N_DRAWS)
    assert abs(float(np.mean(a * b))) <= 4.0 / math.sqrt(N_DRAWS)


@pytest.mark.parametrize("seed", SEEDS)
def test_kolmogorov_smirnov(seed):
    g = np.sort(_draws(seed))
    n = g.size
    cdf = 0.5 * (1.0 + np.frompyfunc(math.erf, 1, 1)(g / math.sqrt(2.0)).astype(np.float64))
    k = np.arange(1, n + 1, dtype=np.float64)
    D = max(float(np.max(k / n - cdf)), float(np.max(cdf - (k - 1) / n)))
    assert math.sqrt(n) * D <= 1.95
