"""Parity of the residence-side kernel (revs_agent_step) with the oracle, through
the C ABI.  Reference: lpsolver.py:44-160 (Home) and 262-284 (loop body)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run_agent(lib, w, pe_old, pe_new, ps, gm, mode, pdhg=None, ydual=None):
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd._lib import HOME_DTYPE, PDHG, check, ptr
    dev = torch.device("cuda:0")
    n, T = w.load.shape
    up = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    d_cost, d_load = up(w.cost), up(w.load)
    d_h = torch.from_numpy(w.homes.view(np.uint8).reshape(n, HOME_DTYPE.itemsize).copy()).to(dev)
    d_peo, d_pen, d_ps, d_gm = up(pe_old), up(pe_new), up(ps), up(gm)
    S = torch.zeros(n, T, dtype=torch.float32, device=dev)
    Cs = torch.zeros(n, T + 1, dtype=torch.float32, device=dev)
    diff = torch.zeros(n, dtype=torch.float32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    part = torch.zeros(n, dtype=torch.float32, device=dev)          # dsq: per-home |dP_sch|^2
    scratch = torch.zeros(3 * lib.revs_residual_num_chunks(n), dtype=torch.float64, device=dev)
    pd = PDHG()
    lib.revs_pdhg_defaults(C.byref(pd))
    for k, v in (pdhg or {}).items():
        setattr(pd, k, v)
    check(lib.revs_agent_step(n, T, ptr(d_cost), ptr(d_h), ptr(d_load), ptr(d_peo), ptr(d_pen),
                              ptr(d_ps), ptr(d_gm), ptr(S), ptr(Cs), ptr(diff), ptr(part),
                              ptr(status), ptr(ydual), w.kappa, _lib.MODES[mode], C.byref(pd),
                              torch.cuda.current_stream().cuda_stream), "agent_step")
    out = torch.zeros(4, dtype=torch.float32, device=dev)
    check(lib.revs_residual_finalize(ptr(diff), ptr(part), n, T, w.kappa, 1e-4, ptr(scratch), ptr(out),
                                     torch.cuda.current_stream().cuda_stream), "finalize")
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().astype(np.float64)
    return dict(P_sch=g(d_ps), G=g(d_gm), S=g(S), C=g(Cs), diff=g(diff), ydual=ydual,
                status=status.cpu().numpy(), resid=g(out), dsq=g(part))


from param_cases import state as _state          # the mid-ADMM state, shared with tests/test_gpu_params.py


def _prep(n, T, seed, **kw):
    from helpers import f32, oracle_homes
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(n, T, seed=seed, n_nodes=16, **kw)
    w.load = f32(w.load)
    w.cost = f32(w.cost)
    return w, oracle_homes(w)


@pytest.mark.parametrize("T,n", [(24, 3001), (96, 3001), (7, 3001), (33, 3001), (130, 3001), (192, 3001), (2, 3001),
                                 (24, 100_000)])
@pytest.mark.parametrize("zero_state", [True, False])
@pytest.mark.parametrize("keys64", [1, 0])
def test_binary_matches_oracle(gpu_lib, T, n, zero_state, keys64):
    """Binary charger = the reference MIQP.  keys64 = 1 (revs_pdhg_t::keys64): the slots' switching costs formed and
    ranked in double in the oracle's order of operations -- the SAME schedule for EVERY residence, exact ties included
    (both sides: earlier slot).  keys64 = 0, the closed loop's default (float keys, formed by the operations that update
    the state: include/revs_admm.h says why): bit-exact wherever the oracle's decision margin exceeds float rounding,
    objective equal everywhere.  (100 000 x 24: BASELINE's headline size, every residence against the oracle.)"""
    from oracle import revs_oracle as ro
    w, oh = _prep(n, T, seed=T)
    if zero_state:
        pe_old = pe_new = ps = gm = np.zeros((n, T))          # lpsolver.py:244-246
    else:
        pe_old, pe_new, ps, gm = _state(w, T)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "binary", dict(keys64=keys64))
    _assert_binary(r, w, oh, (pe_old, pe_new, ps, gm), keys64,
                   ro.home_solve_binary(w.cost, oh, pe_old, ps, gm, w.kappa))


def _g_scale(kappa):
    """G = gm + (kappa/2) check: an error in g reaches G multiplied by kappa/2, so G's absolute tolerance is the one
    set at kappa = 5 times max(1, kappa/5)."""
    return max(1.0, kappa / 5.0)


def _assert_binary(r, w, oh, state, keys64, oracle):
    """What test_binary_matches_oracle asserts of one revs_agent_step launch (r: _run_agent's result; oracle:
    ro.home_solve_binary's on the same inputs).  Shared with tests/test_gpu_params.py."""
    from oracle import revs_oracle as ro
    pe_old, pe_new, ps, gm = state
    p, s, g, st = oracle
    n, T = w.load.shape
    assert ((r["status"] & 0xFF) == st).all()          # same homes flagged infeasible
    assert (st == 0).mean() > (0.9 if T > 4 else 0.3)     # (T = 2: few windows can reach 90 %)
    # the schedule is a set of slots: compare objective (ties / near-ties may pick
    # another slot of equal cost) and exact equality where the choice is unique
    obj_gpu = ro.home_objective(w.cost, oh, r["S"], pe_old, ps, gm, w.kappa)
    obj_ref = ro.home_objective(w.cost, oh, p, pe_old, ps, gm, w.kappa)
    scale = np.maximum(1.0, np.abs(obj_ref))
    assert np.max(np.abs(obj_gpu - obj_ref) / scale) < 2e-5
    same = (np.abs(r["S"] - p).max(axis=1) == 0)
    if keys64:
        assert same.all(), (int((~same).sum()), n)
    else:
        assert same.mean() > 0.995
    # slot counts and window are exact
    assert ((r["S"] > 0).sum(1) == (p > 0).sum(1)).all()
    assert (r["S"][~oh.window()] == 0).all()
    assert np.isin(r["S"], np.concatenate([[0.0], np.unique(w.homes["rating"]).astype(np.float64)])).all()
    # epilogue on the homes with identical schedules: g, SOC, dual update, diff
    chk = pe_new - g
    G = gm + 0.5 * w.kappa * chk
    np.testing.assert_allclose(r["P_sch"][same], g[same], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(r["C"][same], s[same], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(r["G"][same], G[same], rtol=1e-5, atol=1e-5 * _g_scale(w.kappa))
    np.testing.assert_allclose(r["diff"][same], np.linalg.norm(chk, axis=1)[same] / T,
                               rtol=1e-5, atol=1e-6)
    return same


_ORACLE_CACHE = {}


@pytest.mark.parametrize("T,n", [(24, 2003), (96, 2003), (50, 2003), (192, 2003), (24, 10_000), (24, 100_000),
                                 (96, 125_000)])
@pytest.mark.parametrize("mode", ["relaxed_exact", "pdhg", "pdhg_presolve"])
def test_relaxed_matches_oracle(gpu_lib, T, n, mode):
    """Continuous box+SOC QP (north star; n = 10 000 x T = 24 is BASELINE config 1 at its stated
    size).  float32 tolerance: 5e-5 kW absolute on schedules of 3.6-7.2 kW chargers for both solvers
    -- PDHG finishes with the KKT polish on the piece it identified (round 2: 2e-4, PDHG stopping at a
    1e-6 step).  pdhg_presolve: revs_pdhg_t::polish = 3, the KKT steps also BEFORE PDHG -- here from a zero
    multiplier (the cold start: the steps cross many pieces, PDHG takes whatever they leave)."""
    from oracle import revs_oracle as ro
    if n == 125_000 and mode != "pdhg":
        pytest.skip("BASELINE config 4's per-GPU shape: the north star's solver only (the oracle takes ~40 s there)")
    w, oh = _prep(n, T, seed=100 + T, binary_feasible=False)
    pe_old, pe_new, ps, gm = _state(w, T + 1)
    pdhg = None
    if mode == "pdhg_presolve":
        mode, pdhg = "pdhg", dict(polish=3)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode, pdhg)
    # (100 000 x 24 -- the headline size -- and 125 000 x 96: every residence against the oracle, which takes 7 / 40 s
    # there: one run serves the three solvers)
    if (T, n) not in _ORACLE_CACHE:
        if n >= 100_000:
            _ORACLE_CACHE.clear()
        _ORACLE_CACHE[(T, n)] = ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa)
    _assert_relaxed(r, w, (pe_old, pe_new, ps, gm), _ORACLE_CACHE[(T, n)])


def _assert_relaxed(r, w, state, oracle):
    """What test_relaxed_matches_oracle asserts of one revs_agent_step launch (oracle: ro.home_solve_relaxed's on the
    same inputs).  Shared with tests/test_gpu_params.py."""
    pe_old, pe_new, ps, gm = state
    p, s, g, st = oracle
    n, T = w.load.shape
    tol = 5e-5
    assert np.abs(r["S"] - p).max() < tol * max(1.0, w.homes["rating"].max())
    np.testing.assert_allclose(r["C"], s, atol=2e-4)
    chk = pe_new - g
    np.testing.assert_allclose(r["G"], gm + 0.5 * w.kappa * chk, atol=2e-3 * _g_scale(w.kappa), rtol=1e-5)
    np.testing.assert_allclose(r["diff"], np.linalg.norm(chk, axis=1) / T, atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(r["dsq"], ((g - ps) ** 2).sum(axis=1), rtol=2e-3, atol=1e-6)
    # global residuals from the per-home terms (revs_residual_finalize)
    rp = np.sqrt((chk ** 2).sum())
    rd = w.kappa * np.sqrt(((g - ps) ** 2).sum())
    np.testing.assert_allclose(r["resid"][0], rp, rtol=1e-4)
    np.testing.assert_allclose(r["resid"][1], rd, rtol=1e-4)
    np.testing.assert_allclose(r["resid"][2], (np.linalg.norm(chk, axis=1) / T).max(), rtol=1e-4)
    assert r["resid"][3] == 0.0


@pytest.mark.parametrize("full_rows", [0, 1])
def test_pdhg_follows_oracle_iteration(gpu_lib, full_rows):
    """Same PDHG, same step sizes, fixed 64 iterations: kernel vs float32 numpy, for the
    presolved single-row form (default) and the full SOC rows."""
    _assert_pdhg_follows_iteration(gpu_lib, full_rows, 5.0)


def _assert_pdhg_follows_iteration(gpu_lib, full_rows, kappa):
    """test_pdhg_follows_oracle_iteration's check at the ADMM penalty kappa.  Shared with tests/test_gpu_params.py."""
    from oracle import revs_oracle as ro
    n, T = 512, 24
    w, oh = _prep(n, T, seed=7, binary_feasible=False, kappa=kappa)
    pe_old, pe_new, ps, gm = _state(w, 3)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg",
                   dict(max_iter=64, check=64, tol=-1.0, full_rows=full_rows, polish=0))
    p, *_ = ro.home_solve_relaxed_pdhg(w.cost, oh, pe_old, ps, gm, w.kappa, iters=64, tol=0.0,
                                       check=64, dtype=np.float32, full_rows=bool(full_rows))
    assert np.abs(r["S"] - p).max() < 5e-4
    assert ((r["status"] >> 8)[oh.ev] == 64).all()


@pytest.mark.parametrize("T", [24, 96])
def test_pdhg_full_rows_matches_oracle(gpu_lib, T):
    """PDHG with every SOC row kept (full_rows=1) reaches the same optimum."""
    from oracle import revs_oracle as ro
    w, oh = _prep(1500, T, seed=40 + T, binary_feasible=False)
    pe_old, pe_new, ps, gm = _state(w, T)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", dict(full_rows=1))
    p, *_ = ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa)
    assert np.abs(r["S"] - p).max() < 2e-4 * 7.2


def test_no_ev_and_ragged(gpu_lib):
    """Residences without EV keep p = 0, s = 0 (lpsolver.py:70-79); n not a multiple
    of the homes-per-workgroup; a single home."""
    from oracle import revs_oracle as ro
    for n in (1, 5, 33):
        w, oh = _prep(n, 24, seed=n, adoption=0.0)
        z = np.zeros((n, 24))
        r = _run_agent(gpu_lib, w, z, z, z, z, "binary")
        assert (r["S"] == 0).all() and (r["C"] == 0).all()
        np.testing.assert_allclose(r["P_sch"], w.load, rtol=0, atol=0)
        np.testing.assert_allclose(r["G"], -0.5 * w.kappa * w.load, rtol=1e-6)


def test_infeasible_flagged(gpu_lib):
    """A window too short to reach 90% SOC: the reference prints 'No solution found'
    and exits (lpsolver.py:153-155); the kernel flags status 1."""
    w, oh = _prep(64, 24, seed=3)
    w.homes["end"] = w.homes["start"] + 1
    w.homes["nmin"] = np.maximum(w.homes["nmin"], 2)
    w.homes["nmax"] = np.maximum(w.homes["nmax"], w.homes["nmin"])
    z = np.zeros((64, 24))
    r = _run_agent(gpu_lib, w, z, z, z, z, "binary")
    ev = w.homes["ev"].astype(bool)
    assert ((r["status"] & 0xFF)[ev] == 1).all() and ((r["status"] & 0xFF)[~ev] == 0).all()


def test_golden_diff1(gpu_lib, golden):
    """First ADMM iteration on the reference's own feeder data: diff[1] of all 267 EV
    homes equals what the reference stored (out/121144-com2/distributed), to float32."""
    from conftest import golden_homes
    from helpers import f32
    from revs_admm_amd.engine import pack_homes
    from revs_admm_amd.synthetic import Workload
    z, fd = golden
    oh, evi = golden_homes(z, "dis_a90_r4800", 4.8)
    homes = pack_homes(oh.ev, 4.8, 20.0, 0.2, 11, 23)
    n, T = oh.LOAD.shape
    w = Workload(f32(z["tariff_shift6"]), f32(oh.LOAD), homes, np.arange(n), np.eye(2), None, None,
                 1.03, 0.95, 1.05, 5.0)
    zero = np.zeros((n, T))
    r = _run_agent(gpu_lib, w, zero, zero, zero, zero, "binary")
    ref = z["dis_a90_r4800_diff"][:, 0]
    np.testing.assert_allclose(r["diff"][evi], ref, rtol=2e-6)


def test_pdhg_warm_start(gpu_lib):
    """With the multipliers and the previous schedule as the starting point the kernel
    reaches the same optimum in fewer PDHG iterations (the tail below the float32
    stopping tolerance still has to be walked, so the saving is the approach phase)."""
    import torch
    from oracle import revs_oracle as ro
    n, T = 4096, 24
    w, oh = _prep(n, T, seed=21, binary_feasible=False)
    pe_old, pe_new, ps, gm = _state(w, 5)
    cold = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg")
    yd = torch.zeros(n, dtype=torch.float32, device="cuda:0")        # one multiplier per home
    first = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", ydual=yd)
    # same problem again, now starting from its own solution and multipliers
    again = _run_agent(gpu_lib, w, pe_old, pe_new, first["P_sch"], gm, "pdhg", ydual=yd)
    p, *_ = ro.home_solve_relaxed(w.cost, oh, pe_old, first["P_sch"], gm, w.kappa)
    assert np.abs(again["S"] - p).max() < 2e-4 * 7.2
    it_cold = (cold["status"] >> 8)[oh.ev].mean()
    it_warm = (again["status"] >> 8)[oh.ev].mean()
    assert it_warm < 0.95 * it_cold, (it_cold, it_warm)
    # polish bit 1: the KKT steps from the carried multiplier come first; near a solution's own multiplier they
    # settle (nearly) every residence -- PDHG is not entered for those, the schedule is the same optimum
    yd3 = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    first3 = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", dict(polish=3), ydual=yd3)
    assert np.abs(first3["S"] - first["S"]).max() < 5e-5 * 7.2
    assert ((first3["status"] & 0xFF) == 0).all()
    again3 = _run_agent(gpu_lib, w, pe_old, pe_new, first3["P_sch"], gm, "pdhg", dict(polish=3), ydual=yd3)
    assert np.abs(again3["S"] - p).max() < 2e-4 * 7.2
    assert ((again3["status"] >> 8)[oh.ev] == 0).mean() > 0.9 and ((again3["status"] & 0xFF) == 0).all()
    # ... and the cold start settles most residences the same way (what is left runs PDHG, then the steps again)
    assert ((first3["status"] >> 8)[oh.ev] == 0).mean() > 0.5


@pytest.mark.parametrize("mode", ["binary", "relaxed_exact", "pdhg", "pdhg_presolve"])
def test_edge_parameters(gpu_lib, mode):
    """Residences the reference would accept but rarely sees: already charged past 90 %
    (no slot needed), windows reaching outside the horizon, one-slot windows, T = 1, 2, 3."""
    from helpers import f32, oracle_homes
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import pack_homes
    from revs_admm_amd.synthetic import Workload
    rng = np.random.default_rng(3)
    for T in (1, 2, 3, 24):
        n = 96
        ev = np.ones(n, bool)
        ev[::7] = False
        rating = rng.choice([3.6, 7.2], n)
        cap = rng.choice([20.0, 60.0], n)
        init = rng.choice([0.05, 0.5, 0.91, 0.97], n)
        start = rng.integers(-3, max(T - 1, 1), n)
        end = start + rng.integers(1, T + 6, n)
        homes = pack_homes(ev, rating, cap, init, start, end)
        load = f32(rng.uniform(0.2, 5, (n, T)))
        cost = f32(rng.uniform(0.05, 0.3, T))
        w = Workload(cost, load, homes, np.zeros(n, np.int64), np.eye(1), None, None, 1.0, 0.95,
                     1.05, 5.0)
        oh = oracle_homes(w)
        pe_old, pe_new, ps, gm = _state(w, T)
        if mode == "pdhg_presolve":        # (the KKT steps first, from a zero multiplier: revs_pdhg_t::polish = 3)
            r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, "pdhg", dict(polish=3))
        else:
            r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode, dict(keys64=1) if mode == "binary" else None)
        solve = ro.home_solve_binary if mode == "binary" else ro.home_solve_relaxed
        p, s, g, st = solve(w.cost, oh, pe_old, ps, gm, w.kappa)
        assert ((r["status"] & 0xFF) == st).all()
        ok = st == 0
        if mode == "binary":
            obj_g = ro.home_objective(w.cost, oh, r["S"], pe_old, ps, gm, w.kappa)
            obj_r = ro.home_objective(w.cost, oh, p, pe_old, ps, gm, w.kappa)
            assert np.max(np.abs(obj_g - obj_r)[ok] / np.maximum(1, np.abs(obj_r[ok]))) < 2e-5
            assert ((r["S"] > 0).sum(1) == (p > 0).sum(1))[ok].all()
            assert (np.abs(r["S"] - p)[ok].max(axis=1) == 0).all()      # (double keys: the oracle's decision, every residence)
        else:
            err = np.abs(r["S"] - p)[ok].max()
            print(f"edge residences, {mode}: max |S - oracle| = {err:.2e} kW")
            assert err < 1e-4
        assert (r["S"][~oh.window()] == 0).all()
        assert (r["S"][~ok] == 0).all()                      # flagged homes get no schedule
        np.testing.assert_allclose(r["C"][ok][:, 0], np.where(oh.ev, oh.initial, 0)[ok], atol=1e-6)


@pytest.mark.parametrize("lanes,T", [(16, 24), (32, 24), (16, 32), (32, 17)])
@pytest.mark.parametrize("mode", ["pdhg", "relaxed_exact", "binary", "pdhg_presolve"])
def test_wide_lane_shapes_match_oracle(gpu_lib, lanes, T, mode):
    """revs_pdhg_t::lanes -- 16 lanes x 2 slots / 32 lanes x 1 slot per residence at T <= 32 (the shapes for a GPU
    that holds few residences: BASELINE config 2's 12 500 per GPU) -- against the oracle at the default shape's
    tolerances: continuous schedules within 5e-5 kW, on/off schedules identical up to equal-cost ties, the dual
    update and diff of lpsolver.py:280-284; and the streaming loop runs on them (kin iterations per launch)."""
    from oracle import revs_oracle as ro
    n = 1501
    w, oh = _prep(n, T, seed=300 + T + lanes, binary_feasible=(mode == "binary"))
    pe_old, pe_new, ps, gm = _state(w, T + lanes)
    extra = {}
    if mode == "pdhg_presolve":            # (the KKT steps in front of PDHG on the wide shapes: their sums cross 16 / 32 lanes)
        mode, extra = "pdhg", dict(polish=3)
    r = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode, dict(lanes=lanes, **extra))
    r0 = _run_agent(gpu_lib, w, pe_old, pe_new, ps, gm, mode)
    if mode == "binary":
        p, s, g, st = ro.home_solve_binary(w.cost, oh, pe_old, ps, gm, w.kappa)
        np.testing.assert_array_equal(r["S"], r0["S"])          # the ranking does not depend on the lane shape
        same = np.isclose(r["S"], p, atol=1e-6).all(axis=1)
        assert same.mean() > 0.995
    else:
        p, s, g, st = ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa)
        assert np.abs(r["S"] - p).max() < 5e-5 * max(1.0, w.homes["rating"].max())
        chk = pe_new - g
        np.testing.assert_allclose(r["G"], gm + 0.5 * w.kappa * chk, atol=2e-3, rtol=1e-5)
        np.testing.assert_allclose(r["diff"], np.linalg.norm(chk, axis=1) / T, atol=1e-4, rtol=1e-4)
    assert gpu_lib.revs_agent_max_inner(T, lanes) == 16 and gpu_lib.revs_agent_max_inner(24, 0) == 32


@pytest.mark.parametrize("lanes", [16, 32])
def test_wide_lane_shapes_in_the_engine(gpu_lib, lanes):
    """The whole loop on the wide shapes: transient, streaming steady state (16 iterations per launch, verdicts by
    blocks) and the binding regime, against the oracle's run (relaxed homes; 5e-4 kW as the long-horizon test)."""
    from helpers import f32, oracle_homes
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(600, 24, n_nodes=60, seed=11, binary_feasible=False, stress=1.02)
    w.load, w.cost = f32(w.load), f32(w.cost)
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder, pdhg={"lanes": lanes})
    e.run_steps(59)
    e.step(write_sc=True)
    assert e.spec_hist[0] > 20 and e._inner == 16
    d_ref, P_ref, S_ref, C_ref = ro.solve_ADMM(oracle_homes(w), w.Rn, w.node_of, w.cost, w.kappa, 60, w.vset, w.vlow, w.vhigh,
                                               mode="relaxed", util_method="dual")
    P, S, Cs = e.result()
    assert np.abs(S - S_ref).max() < 5e-4
    d_last = e.diff.cpu().numpy()[e.inv_perm]
    assert np.abs(d_last - d_ref[59]).max() < 1e-3 * max(1.0, d_ref.max())
