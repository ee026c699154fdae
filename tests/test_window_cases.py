"""tests/window_cases.py on the host: the atlas holds what its docstring lists at one horizon per lane shape, and the
oracle alone meets the conditions tests/test_gpu_windows.py relies on (which residences it flags, the forced
schedule of the residences that need every slot)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_shapes import FULL, MAX_INNER, RAGGED, shape_of  # noqa: E402
import window_cases as wc  # noqa: E402

HORIZONS = RAGGED + FULL


def _case(T):
    from helpers import oracle_homes
    a = wc.atlas_of(T)
    return a, oracle_homes(wc.workload(a)), wc.SHAPES[shape_of(T)]


def test_one_horizon_per_shape():
    assert {shape_of(T) for T in RAGGED} == set(wc.SHAPES) == set(MAX_INNER)
    for T in HORIZONS:
        lpa, spl = wc.SHAPES[shape_of(T)]
        assert lpa * spl >= T
        assert T in FULL or lpa * spl > T, T           # dead lanes or a ragged lane: slots of the shape beyond the horizon


@pytest.mark.parametrize("T", HORIZONS, ids=[f"T{T}-{shape_of(T)}" for T in HORIZONS])
def test_atlas_holds_every_category_and_need(T):
    a, oh, (lpa, spl) = _case(T)
    n = len(a.homes)
    assert n < 1000 and a.load.shape == (n, T) and a.cost.shape == (T,)
    for x in (a.load, a.cost, oh.rating, oh.capacity, oh.initial):
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    assert (a.load > 0.2 - 1e-6).all() and (a.load < 5).all() and len(np.unique(a.cost)) <= 5
    # the same atlas from the same arguments; another load and tariff from another seed
    b = wc.atlas(T, lpa, spl, T)
    assert np.array_equal(a.homes, b.homes) and np.array_equal(a.load, b.load) and np.array_equal(a.cost, b.cost)
    assert not np.array_equal(a.load, wc.atlas(T, lpa, spl, T + 1).load)
    # every 7th record has no EV, and only those
    ev = a.homes["ev"] != 0
    assert np.array_equal(np.flatnonzero(~ev), np.arange(0, n, 7)) and np.array_equal(a.tags["no_ev"], np.arange(0, n, 7))
    # every category (inside_lane where a lane has three slots) and every need class, and every pair of them
    cats = [c for c in wc.CATEGORIES if c != "inside_lane" or spl >= 3]
    for c in cats:
        assert len(a.tags[c]), c
        for need in wc.NEEDS:
            assert len(np.intersect1d(a.tags[c], a.tags[need])), (c, need)
    assert spl >= 3 or not len(a.tags["inside_lane"])
    for k in wc.CATEGORIES + wc.NEEDS:
        assert ev[a.tags[k]].all(), k
    assert np.array_equal(np.sort(np.concatenate([a.tags[k] for k in wc.NEEDS + ("no_ev",)])), np.arange(n))
    assert np.array_equal(np.sort(np.concatenate([a.tags["feasible"], a.tags["infeasible"]])), np.arange(n))
    # the windows are what the categories say
    s, e = a.homes["start"].astype(np.int64), a.homes["end"].astype(np.int64)
    W = np.minimum(e, T) - np.maximum(s, 0)
    assert (W >= 1).all()
    L = wc.live_lanes(T, spl)
    i = a.tags["one_slot"]
    assert (e[i] - s[i] == 1).all()
    for t in [0, T - 1] + [b - 1 for b in wc.boundaries(T, spl)] + wc.boundaries(T, spl):     # both sides of every boundary
        assert (s[i] == t).any(), t
    i = a.tags["lane"]
    assert (s[i] % spl == 0).all() and ((e[i] == s[i] + spl) | (e[i] == T)).all()
    assert {0, L // 2, L - 1} <= set(s[i] // spl)
    i = a.tags["lane_shifted"]
    assert (s[i] % spl == 1 % spl).all() and ((e[i] == s[i] + spl) | (e[i] == T)).all()
    assert len(i) == 0 or {0, L // 2} <= set((s[i] - 1) // spl)
    i = a.tags["inside_lane"]
    assert (s[i] // spl == (e[i] - 1) // spl).all() and (s[i] % spl > 0).all() and (e[i] < np.minimum((s[i] // spl + 1) * spl, T)).all()
    i = a.tags["horizon"]
    assert (s[i] == 0).all() and (e[i] == T).all()
    i = a.tags["outside"]
    assert {(-3, T + 5), (-3, 2), (T - 2, T + 5)} == set(zip(s[i].tolist(), e[i].tolist()))
    i = a.tags["ragged_lane"]
    assert (s[i] == (L - 1) * spl).all() and (e[i] == T).all()
    if T <= 16:                                        # every pair
        have = set(zip(s[ev].tolist(), e[ev].tolist()))
        assert {(x, y) for x in range(T) for y in range(x + 1, T + 1)} <= have
    # the need classes are what pack_homes made of initial, rating and capacity
    nmin, nmax = a.homes["nmin"].astype(np.int64), a.homes["nmax"].astype(np.int64)
    t = a.tags
    assert (nmin[t["nmin0"]] == 0).all() and (oh.initial[t["nmin0"]] > 0.9).all()
    assert (nmin[t["nmin1"]] == 1).all()
    assert (nmin[t["nmin_half"]] == np.maximum(1, W[t["nmin_half"]] // 2)).all()
    assert (nmin[t["nmin_W"]] == W[t["nmin_W"]]).all()
    assert (nmin[t["nmin_W1"]] == W[t["nmin_W1"]] + 1).all() and (nmax[t["nmin_W1"]] >= nmin[t["nmin_W1"]]).all()
    assert (nmax[t["nmax_lt_nmin"]] < nmin[t["nmax_lt_nmin"]]).all()
    assert (nmax[t["feasible"]] >= nmin[t["feasible"]]).all() and (oh.initial >= 0).all() and (oh.initial[ev] < 1).all()
    # the closed loop's variant: the same without the two infeasible classes
    f = wc.atlas(T, lpa, spl, T, feasible_only=True)
    assert not len(f.tags["infeasible"]) and not len(f.tags["nmin_W1"]) and not len(f.tags["nmax_lt_nmin"])
    for c in cats:
        for need in wc.NEEDS[:4]:
            assert len(np.intersect1d(f.tags[c], f.tags[need])), (c, need)
    assert len(f.homes) < 1000 and not (f.homes["ev"][::7] != 0).any()


@pytest.mark.parametrize("T", HORIZONS, ids=[f"T{T}-{shape_of(T)}" for T in HORIZONS])
def test_oracle_meets_the_gpu_tests_conditions(T):
    """On/off chargers: "No solution found" exactly on nmin_W1 and nmax_lt_nmin.  Continuous chargers have no slot counts:
    the relaxation of an nmax_lt_nmin residence (1.33 slots' energy) is feasible wherever the window holds two slots,
    so ro.home_solve_relaxed flags nmin_W1 and the nmax_lt_nmin residences on one-slot windows, and nothing else.
    nmin_W: both solvers charge at full rating on the whole clipped window -- the continuous one short of it by the
    energy that `initial`, rounded to float32 on the feasible side, leaves out (at most that much in any slot)."""
    from oracle import revs_oracle as ro
    from test_gpu_agent import _state
    a, oh, (lpa, spl) = _case(T)
    w = wc.workload(a)
    n = len(a.homes)
    ev = oh.ev
    nmin, nmax = ro.slot_count_bounds(oh)
    assert np.array_equal(nmin, a.homes["nmin"]) and np.array_equal(nmax[ev], a.homes["nmax"][ev])
    W = oh.window().sum(1)
    bad = np.zeros(n, bool)
    bad[a.tags["infeasible"]] = True
    few = np.zeros(n, bool)
    few[a.tags["nmax_lt_nmin"]] = True
    few &= W < 2
    bad_relaxed = few.copy()
    bad_relaxed[a.tags["nmin_W1"]] = True
    assert few.any() and (bad & ~bad_relaxed).any()
    full = a.tags["nmin_W"]
    for zero in (True, False):
        pe_old, _, ps, gm = (np.zeros((n, T)),) * 4 if zero else _state(w, T)
        pb, sb, gb, stb = ro.home_solve_binary(a.cost, oh, pe_old, ps, gm, w.kappa)
        pr, sr, gr, st_r = ro.home_solve_relaxed(a.cost, oh, pe_old, ps, gm, w.kappa)
        assert np.array_equal(stb == 1, bad) and np.array_equal(stb == 0, ~bad)
        assert np.array_equal(st_r == 1, bad_relaxed) and np.array_equal(st_r == 0, ~bad_relaxed)
        for p, st in ((pb, stb), (pr, st_r)):
            assert (p[~oh.window()] == 0).all() and (p[st == 1] == 0).all() and (p[~ev] == 0).all()
        forced = np.where(oh.window()[full], oh.rating[full, None], 0.0)
        assert np.array_equal(pb[full], forced)
        short = forced.sum(1) - ro.energy_bounds(oh)[0][full]            # energy the rounded `initial` leaves out
        assert (short >= 0).all() and (short <= 2.0 ** -23 * oh.capacity[full]).all()
        assert (pr[full] <= forced).all() and (np.abs(pr[full] - forced).max(axis=1) <= short + 1e-9).all()
        assert np.abs(pr[full] - pb[full]).max() < 1e-4
        # charged past 90 %: the on/off charger takes a slot only where that pays, the state of charge never falls
        assert (sb[:, 1:] >= sb[:, :-1]).all() and (sr[:, 1:] >= sr[:, :-1] - 1e-12).all()
