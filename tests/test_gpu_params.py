"""The residence kernel and the closed loop across the parameter grid of tests/param_cases.py: ADMM penalties whose
reciprocal and half are rounded floats (0.8, 3.3, 7 next to the bench's 5), chargers outside the stock ratings and
capacities, the operator's voltage set point up to 1.045.

One launch of revs_agent_step through the C ABI (tests/test_gpu_agent.py's _run_agent and its assertions, imported, not
restated) at n = 1501 -- ragged, no multiple of the residences per workgroup -- and T = 24 (8 lanes x 3 slots), 96
(16 x 6) and 33 (a ragged slot count); then the engine's loop against ro.solve_ADMM on a small synthetic feeder and on
the golden 121144 feeder.  tests/test_param_cases.py pins the inputs on the CPU."""
import functools

import numpy as np
import pytest

import param_cases as pc

pytestmark = pytest.mark.gpu

N = 1501
HORIZONS = (24, 96, 33)
CHARGER_SETS = sorted(pc.CHARGERS)
_CASES, _ORACLE = {}, {}


def _case(T, kappa, chargers, binary):
    """-> (workload, oracle homes) of a grid point, built once (the seeds of test_binary_matches_oracle /
    test_relaxed_matches_oracle)."""
    from helpers import oracle_homes
    key = (T, kappa, chargers, binary)
    if key not in _CASES:
        w = pc.build(N, T, T if binary else 100 + T, chargers, binary, kappa)
        _CASES[key] = (w, oracle_homes(w))
    return _CASES[key]


def _oracle(key, solve):
    """The oracle's answer of a grid point, once for the kernel variants held to it."""
    if key not in _ORACLE:
        _ORACLE[key] = solve()
    return _ORACLE[key]


@pytest.mark.parametrize("keys64", [1, 0])
@pytest.mark.parametrize("zero_state", [True, False])
@pytest.mark.parametrize("chargers", CHARGER_SETS)
@pytest.mark.parametrize("kappa", pc.KAPPAS)
@pytest.mark.parametrize("T", HORIZONS)
def test_binary_matches_oracle_across_parameters(gpu_lib, T, kappa, chargers, zero_state, keys64):
    """test_binary_matches_oracle's assertions: same status, objective within 2e-5, slot counts, window and rating
    values exact; keys64 = 1 the oracle's schedule for every residence, keys64 = 0 (float keys, the closed loop's) for
    more than 99.5 % -- tests/test_param_cases.py shows the float keys' own restatement reaches 100 % on these inputs;
    the epilogue at that test's tolerances, G's absolute one times max(1, kappa / 5)."""
    from oracle import revs_oracle as ro
    from test_gpu_agent import _assert_binary, _run_agent
    w, oh = _case(T, kappa, chargers, True)
    st8 = (np.zeros((N, T)),) * 4 if zero_state else pc.state(w, T)
    pe_old, pe_new, ps, gm = st8
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "binary", dict(keys64=keys64))
    ref = _oracle(("binary", T, kappa, chargers, zero_state),
                  lambda: ro.home_solve_binary(w.cost, oh, pe_old, ps, gm, w.kappa))
    assert (ref[3] == 0).all()
    same = _assert_binary(r, w, oh, st8, keys64, ref)
    print(f"PARAMS binary T={T} kappa={kappa} {chargers} zero={int(zero_state)} keys64={keys64} differ={int((~same).sum())}")


@pytest.mark.parametrize("mode", ["relaxed_exact", "pdhg", "pdhg_presolve"])
@pytest.mark.parametrize("chargers", CHARGER_SETS)
@pytest.mark.parametrize("kappa", pc.KAPPAS)
@pytest.mark.parametrize("T", HORIZONS)
def test_relaxed_matches_oracle_across_parameters(gpu_lib, T, kappa, chargers, mode):
    """test_relaxed_matches_oracle's assertions: schedules within 5e-5 max(1, max rating) kW of ro.home_solve_relaxed,
    SOC, diff, dsq and revs_residual_finalize's outputs as there, G's absolute tolerance times max(1, kappa / 5).  At
    kappa = 0.8 the linear term is six times larger against the quadratic than at 5: PDHG's step sizes and the KKT polish
    run close to an LP."""
    from oracle import revs_oracle as ro
    from test_gpu_agent import _assert_relaxed, _run_agent
    w, oh = _case(T, kappa, chargers, False)
    st8 = pc.state(w, T + 1)
    pe_old, pe_new, ps, gm = st8
    name, pdhg = mode, None
    if mode == "pdhg_presolve":
        mode, pdhg = "pdhg", dict(polish=3)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode, pdhg)
    ref = _oracle(("relaxed", T, kappa, chargers), lambda: ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa))
    assert (ref[3] == 0).all() and ((r["status"] & 0xFF) == 0).all()
    print(f"PARAMS {name} T={T} kappa={kappa} {chargers} S={np.abs(r['S'] - ref[0]).max():.3e} "
          f"G={np.abs(r['G'] - (gm + 0.5 * w.kappa * (pe_new - ref[2]))).max():.3e} "
          f"passes={int((r['status'] >> 8).max())}")
    _assert_relaxed(r, w, st8, ref)


@pytest.mark.parametrize("chargers", CHARGER_SETS)
@pytest.mark.parametrize("kappa", pc.KAPPAS)
def test_pdhg_full_rows_across_parameters(gpu_lib, kappa, chargers):
    """PDHG with every SOC row kept (full_rows = 1) at T = 24: test_pdhg_full_rows_matches_oracle's tolerance, 2e-4 of
    the largest rating."""
    from oracle import revs_oracle as ro
    from test_gpu_agent import _run_agent
    T = 24
    w, oh = _case(T, kappa, chargers, False)
    pe_old, pe_new, ps, gm = pc.state(w, T + 1)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", dict(full_rows=1))
    p = _oracle(("relaxed", T, kappa, chargers), lambda: ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa))[0]
    err = np.abs(r["S"] - p).max()
    print(f"PARAMS full_rows kappa={kappa} {chargers} S={err:.3e}")
    assert err < 2e-4 * w.homes["rating"].max()


@pytest.mark.parametrize("full_rows", [0, 1])
@pytest.mark.parametrize("kappa", [min(pc.KAPPAS), max(pc.KAPPAS)])
def test_pdhg_follows_oracle_iteration_at_the_grid_ends(gpu_lib, kappa, full_rows):
    """test_pdhg_follows_oracle_iteration's check -- 64 fixed iterations against the float32 numpy PDHG, 5e-4 -- at the
    smallest and the largest penalty: a wrong 1 / (kappa rating) or step size shows here before convergence hides it."""
    from test_gpu_agent import _assert_pdhg_follows_iteration
    _assert_pdhg_follows_iteration(gpu_lib, full_rows, kappa)


# ---- closed loops ----------------------------------------------------------------------------------------------------
def _loop_grid():
    return [(k, pc.VSETS[0]) for k in pc.OFF_KAPPAS] + [(pc.KAPPAS[1], v) for v in pc.VSETS[1:]]


@pytest.mark.parametrize("kappa,vset", _loop_grid())
def test_closed_loop_follows_oracle(gpu_lib, kappa, vset):
    """AdmmEngine.run against ro.solve_ADMM, continuous chargers (closed form), 600 residences on 100 nodes, T = 24,
    60 iterations with binding voltage rows (stress = 1.3), at the tolerances of tests/test_gpu_agent.py::
    test_wide_lane_shapes_in_the_engine: schedules within 5e-4 kW, the last diff within 1e-3 max(1, max diff).
    (make_workload scales the line resistances with the voltage band, so another vset changes the magnitudes of R and
    the lower limit the operator works with, not which rows bind.)"""
    from helpers import f32, oracle_homes
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(600, 24, n_nodes=100, seed=11, binary_feasible=False, stress=1.3, kappa=kappa, vset=vset)
    w.load, w.cost = f32(w.load), f32(w.cost)
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="relaxed_exact", feeder=w.feeder)
    diffs = e.run(60)
    d_ref, P_ref, S_ref, C_ref = ro.solve_ADMM(oracle_homes(w), w.Rn, w.node_of, w.cost, w.kappa, 60, w.vset, w.vlow,
                                               w.vhigh, mode="relaxed", util_method="dual")
    P, S, Cs = e.result()
    print(f"PARAMS loop kappa={kappa} vset={vset} S={np.abs(S - S_ref).max():.3e} "
          f"diff={np.abs(diffs[59] - d_ref[59]).max():.3e} d_ref_max={d_ref.max():.3e}")
    assert np.abs(S - S_ref).max() < 5e-4
    assert np.abs(diffs[59] - d_ref[59]).max() < 1e-3 * max(1.0, d_ref.max())


@pytest.mark.parametrize("kappa", pc.OFF_KAPPAS)
def test_golden_feeder_trajectory_at_other_penalties(gpu_lib, golden, feeder_R, kappa):
    """The golden 121144 feeder, free-running on/off chargers (float keys), 15 iterations, set up as tests/
    test_gpu_config4.py::test_golden_feeder_gpu_trajectory.  No trajectory is stored away from kappa = 5, so the oracle
    checks: iteration 1's mean diff over the EV residences equals the oracle's to 1e-5, and at every iteration the GPU's
    mean diff is closer to the oracle's (ties to the earlier slot) than the oracle under its other consistent tie rule
    (later slot) gets -- the width of "the reference's model under some consistent tie rule", 10 % to 13 % (a tie rule
    redrawn every iteration is off by more than 100 %: tests/test_oracle.py)."""
    from conftest import golden_homes
    from helpers import f32
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import AdmmEngine, pack_homes
    z, fd = golden
    oh, evi = golden_homes(z, "dis_a90_r4800", 4.8)
    n, T = oh.LOAD.shape
    cost = f32(z["tariff_shift6"])
    oh.LOAD = f32(oh.LOAD)
    e = AdmmEngine(cost, pack_homes(oh.ev, 4.8, 20.0, 0.2, 11, 23), oh.LOAD, np.arange(n), feeder_R, kappa=kappa,
                   vset=1.03, vlow=0.95, vhigh=1.05, mode="binary")
    d_gpu = e.run(15)[:, evi].mean(1)
    d_tie = []
    for tie in (None, "last"):
        d, *_ = ro.solve_ADMM(oh, feeder_R, np.arange(n), cost, kappa, 15, 1.03, 0.95, 1.05, mode="binary",
                              util_method="dual", home_solver=functools.partial(ro.home_solve_binary, tie=tie))
        d_tie.append(d[:, evi].mean(1))
    width = float(np.abs(d_tie[1] / d_tie[0] - 1).max())
    rel = np.abs(d_gpu / d_tie[0] - 1)
    print(f"PARAMS golden kappa={kappa} mean diff[k] GPU/oracle - 1: max {rel.max():.2e} at iteration {int(rel.argmax()) + 1}, "
          f"oracle's two tie rules apart by {width:.4f}; per iteration {np.round(rel, 5).tolist()}")
    assert rel[0] < 1e-5
    assert rel.max() < width
