"""The inputs of tests/test_gpu_params.py, pinned on the CPU: at every point of the parameter grid the oracle finds
every residence feasible, and the kernel's float ranking keys -- restated in numpy float32 -- take the float64
decision for EVERY residence.  So the GPU test's allowance of 0.5 % differing residences under float keys is one the
inputs themselves never use: if a change to the inputs made it start hiding differences, this file fails first."""
import numpy as np
import pytest

import param_cases as pc
from helpers import oracle_homes
from oracle import revs_oracle as ro

N = 1501


@pytest.mark.parametrize("chargers", sorted(pc.CHARGERS))
@pytest.mark.parametrize("kappa", pc.KAPPAS)
@pytest.mark.parametrize("T", [24, 96])
def test_inputs_feasible_and_float_keys_decide_as_double(T, kappa, chargers):
    w = pc.build(N, T, T, chargers, True, kappa)
    oh = oracle_homes(w)
    ratings, kwh = pc.CHARGERS[chargers]
    ev = oh.ev
    assert set(np.unique(oh.rating[ev])) == {float(np.float32(r)) for r in ratings}       # (records hold float32)
    assert set(np.unique(np.round(oh.capacity[ev] * 24.0 / T, 4))) == set(kwh)
    for st8 in (np.zeros((4, N, T)), pc.state(w, T)):
        pe_old, _, ps, gm = st8
        p, s, g, st = ro.home_solve_binary(w.cost, oh, pe_old, ps, gm, kappa)
        assert (st == 0).all()
        take = pc.float_keys_decision(w, oh, pe_old, ps, gm)
        same = ((p > 0) == take).all(axis=1)
        assert same.all(), (int((~same).sum()), N)
    # the relaxed residences of the same grid point are feasible as well
    wr = pc.build(N, T, 100 + T, chargers, False, kappa)
    ohr = oracle_homes(wr)
    lo, hi = ro.energy_bounds(ohr)
    assert (lo <= hi).all() and (lo <= (ohr.window() * ohr.rating[:, None]).sum(axis=1)).all()


def test_tightest_charger_takes_one_or_two_slots():
    """11 kW on 40 kWh at T = 24: rating / capacity = 0.275, the regime nmin == nmax or nmax == nmin + 0/1 with at
    most 2 slots -- the grid reaches it."""
    w = pc.build(N, 24, 24, "offstock", True, 5.0)
    h = w.homes
    tight = (h["ev"] != 0) & (h["rating"] == np.float32(11.0)) & np.isclose(h["capacity"], 40.0)
    assert tight.sum() > 20
    assert h["nmin"][tight].min() >= 1 and h["nmax"][tight].max() <= 2
    assert (h["nmin"][tight] == h["nmax"][tight]).any()


def test_build_leaves_make_workload_stream_alone():
    """Same feeder, loads, tariff, EV flags and windows as make_workload draws (bench.py's stream)."""
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w0 = make_workload(N, 24, seed=24, n_nodes=16, kappa=3.3)
    w = pc.build(N, 24, 24, "stock", True, 3.3)
    np.testing.assert_array_equal(w.load, f32(w0.load))
    np.testing.assert_array_equal(w.Rn, w0.Rn)
    for f in ("ev", "start", "end"):
        np.testing.assert_array_equal(w.homes[f], w0.homes[f])
    assert w.kappa == 3.3
