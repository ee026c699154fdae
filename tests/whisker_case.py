"""The input of the whisker-limit cases of test_gpu_network.py and test_gpu_study.py."""
from fractions import Fraction

import numpy as np


def datum_on_the_upper_limit():
    """A star feeder of nine rated lines, T = 1, whose largest loading is EXACTLY numpy's upper whisker limit
    q3 + 1.5 (q3 - q1), for quartiles for which the limit with an unrounded product (a fused multiply-add) is lower.
    -> (parent, edge_r, cons_of, p (9, 1), rating, the limit).

    Nine values: the quartiles are the data at ranks 2, 4 and 6; the ninth, the last line in preorder, is the maximum
    and moves none of them.  The injections are multiples of 2^-20 below 4: in a star a line's flow is its node's
    injection, and every partial sum of nine such numbers is exact in whatever order a scan takes them, so the loading
    is the one correctly rounded quotient |flow| / rating that numpy computes too.  The fine bits are in the ratings;
    the last line's rating is found by stepping ulps until that quotient is the limit."""
    rng = np.random.default_rng(1505)
    for _ in range(200):
        f = np.round(rng.uniform(0.5, 2.0, 8) * 2.0 ** 20) / 2.0 ** 20
        r = f / rng.uniform(0.2, 1.3, 8)
        ld = np.sort(f / r)
        q1, q3 = ld[2], ld[6]
        hival = q3 + 1.5 * (q3 - q1)
        if hival <= ld[7] or float(Fraction(q3) + Fraction(3, 2) * Fraction(q3 - q1)) >= hival:
            continue
        f9 = np.round(1.9 * hival * 2.0 ** 20) / 2.0 ** 20       # (rating near 1.9: its ulp is finer than the quotient's)
        r9 = f9 / hival
        for cand in [r9] + [x for k in range(1, 65) for x in (r9 + k * np.spacing(r9), r9 - k * np.spacing(r9))]:
            if f9 / cand == hival:
                M = 9
                p = np.append(f, f9).reshape(M, 1)
                return np.full(M, -1, np.int64), np.full(M, 1e-3), np.arange(M), p, np.append(r, cand), hival
    raise AssertionError("no such sample within 200 draws")
