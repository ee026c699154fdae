"""certificate.ray_search_many: S searches along their rays in lock-step, one batched evaluation per round, against
certificate.ray_search on each function alone (host only)."""
import math

import numpy as np


def _functions():
    """Seven concave piecewise-linear functions min_k(a_k + b_k x) on x >= 0, seeded, shaped by where the maximum lies:
    at 0, inside (0, 1), beyond 1 after 1 / 3 / 6 doublings, +inf at 0 (a problem with empty rows), and one to skip."""
    rng = np.random.default_rng(20)

    def peaked(peak, pieces=6):
        """Tangents of the concave h - c (x - peak)^2 at `peak` and at random points around it: their minimum is
        piecewise linear and concave with its maximum at `peak`."""
        h, c = rng.uniform(-5, 5), rng.uniform(0.5, 2.0) / peak
        xk = np.concatenate([[peak], peak * rng.uniform(0.0, 3.0, pieces)])
        slope = -2.0 * c * (xk - peak)
        return (h - c * (xk - peak) ** 2) - slope * xk, slope

    def at_zero():
        b = -np.sort(rng.uniform(0.1, 2.0, 5))
        return rng.uniform(-3, 3) + rng.uniform(0, 1, 5) * np.arange(5), b

    coefs = [at_zero(), peaked(0.37), peaked(1.7), peaked(11.0), peaked(90.0), peaked(0.6), peaked(2.5)]
    inf_at_zero = 5

    def make(k):
        a, b = coefs[k]

        def f(x):
            if k == inf_at_zero:
                return math.inf, 2
            return float(np.min(a + b * x)), 0
        return f
    return [make(k) for k in range(7)], np.array([False] * 6 + [True])


def _scalar(f):
    """ray_search on f alone -> ((s, value, empty), scales in order of evaluation)."""
    from revs_admm_amd.certificate import ray_search
    asked = []

    def phi(x):
        asked.append(x)
        return f(x)
    return ray_search(phi), asked


def _doublings(asked):
    """Evaluations of the doubling phase: the scales 2, 4, 8, ... asked right after 0 and 1."""
    k = 0
    while 2 + k < len(asked) and asked[2 + k] == 2.0 ** (k + 1):
        k += 1
    return k


def _many(fs, skip=None):
    from revs_admm_amd.certificate import ray_search_many
    S = len(fs)
    asked = [[] for _ in range(S)]

    def phi_many(scales):
        assert scales.shape == (S,)
        out = [f(float(x)) for f, x in zip(fs, scales)]
        for s in range(S):
            asked[s].append(float(scales[s]))
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])
    return ray_search_many(phi_many, S, skip=skip), asked


def test_the_functions_cover_every_shape_of_search():
    fs, skip = _functions()
    res = [_scalar(f) for f in fs]
    (r0, a0), (r1, a1) = res[0], res[1]
    assert r0[0] == 0.0 and _doublings(a0) == 0                       # maximum at 0
    assert 0.0 < r1[0] < 1.0                                          # inside (0, 1)
    dbl = [_doublings(a) for _, a in res[2:5]]
    assert all(r[0] > 1.0 for r, _ in res[2:5]) and min(dbl) >= 1 and max(dbl) >= 5 and len(set(dbl)) == 3, dbl
    assert res[5][0] == (0.0, math.inf, 2) and res[5][1] == [0.0, 1.0]    # +inf at 0: nothing to search
    for (s, v, _), a in res[:5]:                                      # (each maximum is found to the bracket's width)
        assert len(a) == len(set(a)) and len(a) <= 2 + _doublings(a) + 48


def test_lockstep_search_equals_every_scalar_search():
    fs, skip = _functions()
    (s, v, e, rounds), asked = _many(fs, skip)
    want = [_scalar(f) for f in fs]
    for k in range(len(fs)):
        if skip[k]:
            assert (s[k], v[k], e[k]) == (0.0, *fs[k](0.0))
            assert set(asked[k]) == {0.0}
            continue
        (ws, wv, we), wa = want[k]
        assert s[k] == ws and v[k] == wv and e[k] == we, (k, s[k], ws, v[k], wv)
        # its distinct scales, in order of first appearance, are the scalar search's sequence
        assert list(dict.fromkeys(asked[k])) == wa, k
    assert all(len(a) == rounds for a in asked)
    longest = max(len(wa) for (_, wa), sk in zip(want, skip) if not sk)
    assert rounds == longest
    assert rounds <= 2 + max(_doublings(wa) for _, wa in want) + 48
    assert rounds < sum(len(wa) for _, wa in want)


def test_one_scenario_degenerates_to_the_scalar_search():
    fs, _ = _functions()
    for f in fs[:6]:
        (s, v, e, rounds), asked = _many([f])
        (ws, wv, we), wa = _scalar(f)
        assert (s[0], v[0], e[0]) == (ws, wv, we) and asked[0] == wa and rounds == len(wa)
    (s, v, e, rounds), asked = _many([fs[2]], skip=[True])
    assert (s[0], v[0], rounds) == (0.0, fs[2](0.0)[0], 1) and asked[0] == [0.0]


def test_ties_go_to_the_smaller_scale():
    """max(seen, key=(value, -scale)): on a plateau from 0 on the search stays at 0, alone and in lock-step."""
    from revs_admm_amd.certificate import ray_search, ray_search_many
    assert ray_search(lambda x: (1.0, 0)) == (0.0, 1.0, 0)
    s, v, e, rounds = ray_search_many(lambda x: (np.ones(2), np.zeros(2, int)), 2)
    assert s.tolist() == [0.0, 0.0] and v.tolist() == [1.0, 1.0] and rounds == 27
