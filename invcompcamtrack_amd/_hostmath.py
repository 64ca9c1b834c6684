"""Private helpers that more than one host restatement needs, each stated once: the counter-based draw stream of
csrc/ictr_draw_hd.h, IEEE division for Python floats and the library's f64 exp map."""
from __future__ import annotations

import math

import numpy as np

from ._lib import dp, f64c, load

M64 = (1 << 64) - 1
MAX_DRAWS = 1024    # kRanMaxDraws


def mix(z):
    """splitmix64 (ran_mix)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_indices_n(seed, t, n, count, max_draws=MAX_DRAWS):
    """The first `count` distinct indices of trial t's stream (draw order); fewer than `count` (a shorter list) when
    max_draws draws do not give them. ransac.draw_indices is this with count = 4."""
    sm = mix(int(seed) & M64)
    out = []
    for k in range(max_draws):
        u = mix(sm ^ (((int(t) << 32) | k) & M64))
        i = ((u >> 32) * int(n)) >> 32
        if i not in out:
            out.append(i)
            if len(out) == count:
                break
    return out


def div(a, b):
    """a / b as IEEE 754 has it (no ZeroDivisionError)."""
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def se3_exp_d(p):
    """[R | t] = exp(p), (3, 4) f64, by the library's exp map."""
    G = np.empty(12, np.float64)
    load().ictr_se3_coeff_to_group_d(dp(G), dp(f64c(p)))
    return G.reshape(3, 4)
