"""The numpy restatement of the rule schedules (tests/rules_ref.py) on the host: its schedules respect each residence's
own rows, agree with the oracle's individual optimum where that optimum IS a rule schedule (an anchor that shares no code
with the restatement), and never cost less than the residence's own minimum (tests/bound_ref.py).  No GPU."""
import numpy as np
import pytest

import bound_ref
import rules_ref as rr

T = 24


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    homes = rr.records(rng, 400, T)
    load = rng.uniform(0.1, 3.0, (len(homes), T)).astype(np.float32)
    return homes, load


def exact_f32_records(rng, n, T):
    """Random records whose rating / capacity / initial are float32 values already: the record's nmin / nmax (computed
    from the inputs in double) and the oracle's (computed from the record's fields) come from the same numbers."""
    from revs_admm_amd.engine import pack_homes
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    start = rng.integers(-2, T + 1, n)
    return pack_homes(rng.random(n) < 0.8, f(rng.choice([1.2, 3.3, 4.8, 7.2, 11.5], n)), f(rng.uniform(10.0, 80.0, n)),
                      f(rng.uniform(0.05, 0.98, n)), start, start + rng.integers(0, T + 4, n))


@pytest.mark.parametrize("policy, fill, integral", rr.combos())
def test_schedules_respect_the_residences_own_rows(case, policy, fill, integral):
    homes, load = case
    p, soc, g, status = rr.rule_schedule(homes, load, policy, fill, integral)
    assert p.dtype == soc.dtype == g.dtype == np.float32 and status.dtype == np.int32
    assert p.shape == (len(homes), T) and soc.shape == (len(homes), T + 1) and set(np.unique(status)) <= {0, 1}
    t = np.arange(T)[None, :]
    win = (homes["ev"] != 0)[:, None] & (t >= homes["start"][:, None]) & (t < homes["end"][:, None])
    assert (p[~win] == 0).all()                                  # nothing outside the window, nothing without an EV
    assert (p >= 0).all() and (p <= homes["rating"][:, None]).all()
    assert np.array_equal(g, load + p)
    ok = (status == 0) & (homes["ev"] != 0)
    assert ok.sum() > 20 and (status == 1).sum() > 5
    P = rr.plan(homes, T, policy, fill, integral)
    W = np.maximum(np.clip(homes["end"], 0, T) - np.clip(homes["start"], 0, T), 0)
    rating = homes["rating"].astype(np.float64)
    if integral:
        # k slots at the rating -- the whole window where it holds fewer (status 0: still nmin or more)
        want = np.minimum(P["E_want"], W)
        got = (p == homes["rating"][:, None]).sum(1) * (rating > 0) + want * (rating == 0)
        assert np.array_equal(got[ok], want[ok])
        assert ((p == 0) | (p == homes["rating"][:, None])).all()
        assert (want[ok] >= homes["nmin"][ok]).all() and (want[ok] <= homes["nmax"][ok]).all()
    else:
        # E delivered -- the window's capacity rating W where that is less; one float32 rounding per slot
        want = np.minimum(P["E_want"], rating * W)
        got = p.astype(np.float64).sum(1)
        assert (np.abs(got - want)[ok] <= 2.0 ** -23 * want[ok] + 1e-12).all()
        ini, cap = homes["initial"].astype(np.float64), homes["capacity"].astype(np.float64)
        assert (want[ok] >= ((np.maximum(0.9, ini) - ini) * cap)[ok]).all() and (want[ok] <= ((1.0 - ini) * cap)[ok]).all()
    # the state of charge follows the powers, ends where the energy says, and never falls
    rec = rr.soc_recurrence(homes, p)
    assert np.abs(soc - rec).max() <= 1e-6
    assert (np.diff(soc.astype(np.float64), axis=1) >= 0).all()
    assert (soc[homes["ev"] == 0] == 0).all()
    served = ok & (rating > 0)          # (the edge record with rating 0 has its slot counts set by hand: nmin = 0)
    assert (soc[served, -1] >= 0.9 - 1e-6).all() and (soc[:, -1] <= 1.0 + 1e-6)[homes["nmax"] >= 0].all()


@pytest.mark.parametrize("shape, policy", [("increasing", rr.ASAP), ("flat", rr.ASAP), ("decreasing", rr.ALAP)])
def test_oracle_individual_optimum_is_the_rule_schedule_on_monotone_tariffs(shape, policy):
    """oracle.solve_residence takes the min(nmax, W) cheapest window slots while 0.01 c_t < 0.99 / capacity, ties to the
    earlier slot: the first ones under an increasing or a flat tariff, the last ones under a decreasing one -- the
    ASAP / ALAP schedule of on/off chargers filled to 100 %.  (A record with nmin > nmax has empty rows under the
    contract; the individual mode has no s_T >= 0.9 row and never sees nmin: such records are left out.)"""
    from oracle import revs_oracle as ro
    rng = np.random.default_rng(5)
    homes = exact_f32_records(rng, 300, T)
    homes = homes[homes["nmin"] <= homes["nmax"]]
    assert len(homes) > 200 and (homes["ev"] != 0).sum() > 100
    load = rng.uniform(0.1, 3.0, (len(homes), T))
    tariff = {"increasing": np.linspace(0.05, 0.9, T), "flat": np.full(T, 0.3), "decreasing": np.linspace(0.9, 0.05, T)}[shape]
    assert (0.01 * tariff.max() < 0.99 / homes["capacity"].astype(np.float64)).all()
    p_or = ro.solve_residence(tariff, ro.homes_from_records(load, homes))[0]
    p, _, _, status = rr.rule_schedule(homes, load.astype(np.float32), policy, rr.FULL, 1)
    assert p_or.any() and np.array_equal(p_or, p.astype(np.float64))
    on = (p_or > 0).sum(1)
    assert (on[homes["rating"] > 0] > 0).any() and (on <= np.maximum(homes["nmax"], 0)).all()


@pytest.mark.parametrize("policy, fill, integral", rr.combos())
def test_a_served_schedule_costs_no_less_than_the_residences_minimum(case, policy, fill, integral):
    """A rule schedule with status 0 lies in the residence's feasible set X_h: c . g_h >= min over X_h of c . g_h, the
    residences' part of the dual bound without multipliers."""
    homes, load = case
    rng = np.random.default_rng(3)
    cost = rng.uniform(-0.05, 0.4, T).astype(np.float32)
    p, soc, g, status = rr.rule_schedule(homes, load, policy, fill, integral)
    ok = status == 0
    h, l = homes[ok], load[ok]
    bound, parts, n_empty, p_min, _ = bound_ref.dual_bound(cost, h, l, np.zeros(len(h), np.int64), np.zeros((1, 1)), None,
                                                           1.0, -0.1, 0.1, integral=bool(integral))
    assert n_empty == 0                                          # (status 0: the residence's own rows are not empty)
    c = cost.astype(np.float64)
    mine, least = p[ok].astype(np.float64) @ c, p_min @ c
    assert (mine >= least - 1e-6 * np.maximum(1.0, np.abs(least))).all()
    total = (g[ok].astype(np.float64) @ c).sum()
    assert total >= bound - 1e-6 * abs(bound) and (mine > least + 1e-3).any()
