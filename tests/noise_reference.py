"""numpy restatement of the noise generator of add_noise (normal_pair and mix64 in ac_internal.h), written from its rules.

The generator is counter-based: element e of the flattened tensor depends on (seed, e) only.

1. The seed is taken modulo 2^64 (a negative seed and its 64-bit image give one stream).  key = mix64(seed).
2. mix64 is splitmix64's output function on uint64 with wrap-around arithmetic:
   z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
   z ^= z >> 31.
3. Pair p draws r = mix64(key ^ p):  u1 = ((r >> 40) + 1) / 2^24 in (0, 1],  u2 = ((r >> 8) & 0xFFFFFF) / 2^24 in [0, 1).
4. Box-Muller:  R = sqrt(-2 ln u1),  theta = 2 pi u2.
5. Element e belongs to pair p = e >> 1:  e = 2 p takes R cos(theta),  e = 2 p + 1 takes R sin(theta).

Everything after the integer part is float64 here; the kernel's float32 transcendentals differ from it by their own error.
add_noise returns X + thr * g / 6 with g these standard normals.
"""

import math

import numpy as np

MASK64 = (1 << 64) - 1


def mix64(z):
    """Rule 2 on a uint64 array (or scalar)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, pairs):
    """Rules 1 and 3: (u1, u2) of the pair indices ``pairs`` (uint64 array), exact in float64."""
    key = mix64(np.uint64(int(seed) & MASK64))
    r = mix64(key ^ np.asarray(pairs, dtype=np.uint64))
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return u1, u2


def normal_pair(seed, pairs):
    """Rules 3 and 4: (R cos(theta), R sin(theta)) of the pair indices ``pairs``, float64."""
    u1, u2 = uniforms(seed, pairs)
    rad = np.sqrt(-2.0 * np.log(u1))
    theta = 2.0 * math.pi * u2
    return rad * np.cos(theta), rad * np.sin(theta)


def normals(seed, n, first=0):
    """Rule 5: the standard normals of elements first ... first + n - 1 of a flattened tensor, float64 [n]."""
    p0, p1 = first >> 1, (first + n + 1) >> 1
    c, s = normal_pair(seed, np.arange(p0, p1, dtype=np.uint64))
    g = np.empty(2 * (p1 - p0), dtype=np.float64)
    g[0::2] = c
    g[1::2] = s
    lo = first - 2 * p0
    return g[lo:lo + n]
