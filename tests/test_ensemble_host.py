"""The ensemble's host side (revs_admm_amd/ensemble.py, lpsolver.solve_ADMM_many): limits, argument checks and how
scenarios are cut into ensembles.  Everything here is decided before the device is touched.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(n, seed=0):
    from revs_admm_amd.engine import pack_homes
    rng = np.random.default_rng(seed)
    return pack_homes(rng.random(n) < 0.5, 4.8, 20.0, 0.2, 11, 23)


def test_the_column_limit_is_the_headers():
    from revs_admm_amd import _lib, ensemble  # noqa: F401  (the module imports without a GPU)
    text = open(os.path.join(ROOT, "include", "revs_admm_ops.h")).read()
    assert _lib.ENS_MAX_COLS == 1024 == int(re.search(r"#define\s+REVS_ENS_MAX_COLS\s+(\d+)", text).group(1))
    text = open(os.path.join(ROOT, "include", "revs_admm.h")).read()
    assert _lib.MAX_T == int(re.search(r"#define\s+REVS_MAX_T\s+(\d+)", text).group(1))
    # the new define lives in the operator's header: the boundary stays as tests/test_abi.py holds it
    assert "REVS_ENS_MAX_COLS" not in text


@pytest.mark.parametrize("S,T,ok", [(41, 25, False), (1025, 1, False), (42, 24, True), (43, 24, False), (10, 96, True),
                                    (11, 96, False), (5, 193, False), (1, 192, True)])
def test_columns_beyond_the_limit_raise(S, T, ok):
    """S T = 1025 (41 x 25, 1025 x 1) and every other shape past REVS_ENS_MAX_COLS or REVS_MAX_T: ValueError."""
    from revs_admm_amd.ensemble import AdmmEnsemble, check_shape
    if ok:
        check_shape(S, T)
        return
    with pytest.raises(ValueError):
        check_shape(S, T)
    n = 6
    with pytest.raises(ValueError):          # ... from the constructor, before it looks for a device
        AdmmEnsemble(np.ones(T), [_records(n, s) for s in range(S)], np.ones((n, T)), np.zeros(n, np.int64), np.eye(1),
                     device="cuda:0")


def test_a_process_group_raises():
    from revs_admm_amd.ensemble import AdmmEnsemble
    n, T = 6, 24
    with pytest.raises(NotImplementedError, match="one GPU"):
        AdmmEnsemble(np.ones(T), [_records(n), _records(n, 1)], np.ones((n, T)), np.zeros(n, np.int64), np.eye(1),
                     group=object())


def test_scenarios_over_different_residences_raise():
    from revs_admm_amd.ensemble import AdmmEnsemble
    n, T = 6, 24
    args = (np.zeros(n, np.int64), np.eye(1))
    with pytest.raises(ValueError, match="same residences"):
        AdmmEnsemble(np.ones(T), [_records(n), _records(n + 1)], np.ones((n, T)), *args)
    with pytest.raises(ValueError, match="same residences"):
        AdmmEnsemble(np.ones(T), [_records(n), np.zeros(n)], np.ones((n, T)), *args)
    with pytest.raises(ValueError, match="load has shape"):
        AdmmEnsemble(np.ones(T), [_records(n), _records(n)], np.ones((3, n, T)), *args)
    with pytest.raises(ValueError, match="empty"):
        AdmmEnsemble(np.ones(T), [], np.ones((n, T)), *args)


def _graph(n_res):
    import networkx as nx
    g = nx.Graph()
    g.add_node(0, label="S")
    for i in range(1, n_res + 1):
        g.add_node(i, label="H")
        g.add_edge(i - 1, i, r=0.01)
    return g


def test_solve_many_checks_every_scenarios_residences():
    """A scenario that lacks a residence of the graph: KeyError naming it; LOADs of another length: ValueError -- both
    before any engine is built."""
    from revs_admm_amd.lpsolver import solve_ADMM_many
    g, T = _graph(4), 24
    full = {h: {"LOAD": [1.0] * T, "EV": {}} for h in range(1, 5)}
    short = {h: full[h] for h in (1, 2, 3)}
    with pytest.raises(KeyError, match="scenario 1.*residence 4"):
        solve_ADMM_many([full, short], g, [1.0] * T)
    longer = {h: {"LOAD": [1.0] * (T + 1), "EV": {}} for h in range(1, 5)}
    with pytest.raises(ValueError, match="scenario 1"):
        solve_ADMM_many([full, longer], g, [1.0] * T)
    assert solve_ADMM_many([], g, [1.0] * T) == []


def test_how_scenarios_are_cut_into_ensembles():
    """36 scenarios: one ensemble at T = 24 (at most 42 fit), four of at most 10 at T = 96; the parts tile 0..S in
    order and differ in size by at most one."""
    from revs_admm_amd.lpsolver import split_scenarios
    assert split_scenarios(36, 24) == [(0, 36)]
    assert split_scenarios(36, 96) == [(0, 9), (9, 18), (18, 27), (27, 36)]
    assert split_scenarios(0, 24) == [] and split_scenarios(1, 192) == [(0, 1)]
    for T in (1, 7, 24, 32, 96, 192):
        cap = 1024 // T
        for S in (1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 36, 100):
            if S < 1:
                continue
            parts = split_scenarios(S, T)
            sizes = [b - a for a, b in parts]
            assert parts[0][0] == 0 and parts[-1][1] == S and all(p[1] == q[0] for p, q in zip(parts, parts[1:]))
            assert max(sizes) <= cap and max(sizes) - min(sizes) <= 1 and len(parts) == -(-S // cap), (S, T)
    with pytest.raises(ValueError):
        split_scenarios(3, 193)


def test_study_passes_its_distributed_scenarios_on_together(golden, monkeypatch):
    """REVS.study(ensemble=True): the grid's distributed scenarios reach solve_ADMM_many in one call, in grid order, with
    get_distributed_optimal's keywords; labels and the order of the profiles are those of ensemble=False."""
    import study_ref as sr
    from test_network_host import golden_graph
    from revs_admm_amd import revs_fixture, study
    from revs_admm_amd.revs_fixture import REVS
    z, _ = golden
    monkeypatch.setattr(study, "native_study", sr.host_study)
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], z["LOAD"])}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = z["tariff_shift6"].tolist()
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    calls = []

    def schedule(homes, scale):
        return {h: (np.array(homes[h]["LOAD"]) + (scale if homes[h]["EV"] else 0.0)).tolist() for h in res}

    def many(homes_list, graph, cost, grbpath=None, **kw):
        calls.append((len(homes_list), kw))
        return [(None, schedule(h, 0.25), None, None) for h in homes_list]

    def one(self, tariff, homes, dist, save=False, **kw):
        return schedule(homes, 0.25), None, None

    def individual(self, tariff, homes, save=False, **kw):
        return schedule(homes, 1.0), None, None

    monkeypatch.setattr(revs_fixture, "solve_ADMM_many", many)
    monkeypatch.setattr(REVS, "get_distributed_optimal", one)
    monkeypatch.setattr(REVS, "get_individual_optimal", individual)
    fx = REVS(device="cpu")
    grid = dict(adoptions=(30, 90), ratings=(4800,), seeds=(1234, 56), group_by=("method", "adoption"), arrays=True,
                max_iterations=7, v0=1.03)
    lab0, rep0 = fx.study(tariff, all_homes, dist, com, **grid)
    assert calls == []
    lab1, rep1 = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)
    assert len(calls) == 1 and calls[0][0] == 4
    assert calls[0][1]["iter_max"] == 7 and calls[0][1]["vset"] == 1.03 and calls[0][1]["mode"] == "binary"
    assert lab1 == lab0 and rep1.node_p.tobytes() == rep0.node_p.tobytes()
    assert rep1.groups.tolist() == rep0.groups.tolist()


def test_the_driver_on_the_host_stand_in_follows_the_oracle():
    """The ensemble's driver -- both views of the state, the sort by node, the records [n][S], run / result / get_state /
    set_state -- over the numpy stand-in of the kernels (tests/fake_kernels.py; the Python Newton loop): three scenarios
    that differ in EV ownership, rating and (one) load, each against its own oracle run at the single engine's bars.
    The kernels themselves are tests/test_gpu_ensemble.py's job."""
    from fake_kernels import FakeKernels
    from helpers import f32
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(150, 24, n_nodes=15, seed=11, binary_feasible=False, stress=1.4)
    w.load, w.cost = f32(w.load), f32(w.cost)
    rng = np.random.default_rng(5)
    n, T, S, iters = 150, 24, 3, 5
    capacity, start, end = rng.choice([20.0, 40.0, 60.0], n), rng.integers(10, 14, n), rng.integers(21, 25, n)
    homes = []
    for s, rating in enumerate((3.6, 4.8, 7.2)):
        ev = rng.random(n) < (0.3, 0.5, 0.7)[s]
        initial = np.maximum(np.clip(0.9 - rng.uniform(0.3, 0.7, n), 0.05, 0.85), 0.9 - 0.9 * rating / capacity * (end - start - 1))
        homes.append(pack_homes(ev, rating, capacity, initial, start, end))
    load = np.stack([w.load] * S)
    load[1] = f32(w.load * rng.uniform(0.8, 1.2, w.load.shape))
    e = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                     mode="relaxed_exact", device="cpu", _kernels=FakeKernels())
    assert (e.n, e.T) == (n, S * T) and e.op.speculate is False and e.op.chain is False
    d = e.run(iters)
    P, Sc, Cs = e.result()
    assert d.shape == (S, iters, n) and P.shape == Sc.shape == (S, n, T) and Cs.shape == (S, n, T + 1)
    assert set(e.op_path_hist) == {"dual"} and max(nw for nw, _, _ in e.newton_hist) >= 1
    for s in range(S):
        d_ref, P_ref, S_ref, C_ref = ro.solve_ADMM(ro.homes_from_records(load[s], homes[s]), w.Rn, w.node_of, w.cost, w.kappa,
                                                   iters, w.vset, w.vlow, w.vhigh, mode="relaxed", util_eps=1e-10)
        assert np.abs(d[s] - d_ref).max() < 1e-3 * max(1.0, d_ref.max()), s
        assert np.abs(Sc[s] - S_ref).max() < 2e-5 and np.abs(P[s] - P_ref).max() < 2e-5 and np.abs(Cs[s] - C_ref).max() < 5e-6, s
    assert np.abs(Sc[0] - Sc[2]).max() > 0.1                         # no broadcast
    # one scenario's state out and in: the others are left alone
    before = [e.get_state(s) for s in range(S)]
    e.set_state(1, *[2.0 * a for a in before[1]])
    for s in (0, 2):
        assert all(np.array_equal(a, b) for a, b in zip(e.get_state(s), before[s]))
    assert all(np.array_equal(a, f32(2.0 * b)) for a, b in zip(e.get_state(1), before[1]))
    assert e.multipliers(0).shape == (15, T)
    with pytest.raises(NotImplementedError):
        e.network_report()
    # reset(): every scenario back to iteration 0, the same run again
    e.reset()
    assert e.iteration == 0 and e.op_path_hist == [] and float(e.yd[0].abs().max()) == 0.0
    assert np.array_equal(e.run(iters), d) and all(np.array_equal(a, b) for a, b in zip(e.result(), (P, Sc, Cs)))


class _Recorder:
    """FakeKernels behind a note of every call: (entry, its row count -- the argument named n or m -- and its T, None
    where the entry has none, (engine.n, engine.T) at the time of the call)."""

    def __init__(self, kernels):
        self._kernels, self.engine, self.calls = kernels, None, []

    def __getattr__(self, name):
        import inspect
        fn = getattr(self._kernels, name)
        sig = inspect.signature(fn)

        def entry(*a, **k):
            b = sig.bind(*a, **k).arguments
            e = self.engine
            self.calls.append((name, (b.get("n", b.get("m")), b.get("T")), (getattr(e, "n", None), getattr(e, "T", None))))
            return fn(*a, **k)
        return entry


def test_every_call_carries_its_own_shape_and_nothing_swaps():
    """The engine's two named shapes (engine.py, _init_residences) on the host stand-in: the calls that pass residence-side
    buffers carry the sweep shape, the operator's and the node sums' calls (M, T), and (e.n, e.T) is the same at every
    call -- for an ensemble of S = 3 and for a plain engine on its scenario 0."""
    from fake_kernels import FakeKernels
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine, pack_homes
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    n, T, S, M = 150, 24, 3, 15
    w = make_workload(n, T, n_nodes=M, seed=11, binary_feasible=False, stress=1.4)
    w.load, w.cost = f32(w.load), f32(w.cost)
    rng = np.random.default_rng(5)
    homes = [pack_homes(rng.random(n) < share, 4.8, 20.0, 0.2, 11, 23) for share in (0.3, 0.5, 0.7)]
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="relaxed_exact", device="cpu")

    def recorded(make, sweep, state):
        rec = _Recorder(FakeKernels())
        e = rec.engine = make(rec)
        assert (e.sweep_n, e.sweep_T) == sweep and (e.n, e.T) == state
        e.run(3)
        e.residuals()
        e.result()
        e.reset()
        e.run(2)
        assert (e.sweep_n, e.sweep_T) == sweep and (e.n, e.T) == state
        by = lambda *prefixes: [c for c in rec.calls if c[0].startswith(prefixes)]
        sweeps, finals = by("revs_agent_step"), by("revs_residual_finalize")
        assert len(sweeps) >= 5 and len(by("revs_agent_step_out")) >= 1 and len(finals) >= 1
        assert all(c[1] == sweep for c in sweeps + finals)
        assert [c[1] for c in by("revs_residual_num_chunks")] == [(sweep[0], None)]
        node_side = by("revs_op_dual_", "revs_aggregate_")
        assert by("revs_op_dual_") and all(c[1][0] in (None, M) and c[1][1] in (None, state[1]) and c[1] != (None, None)
                                           for c in node_side)
        # every call of the constructed engine, the sweeps among them: nothing swaps n and T
        after = [c for c in rec.calls if c[2] != (None, None)]
        assert all(c in after for c in sweeps + finals) and all(c[2] == state for c in after)
        return rec

    recorded(lambda k: AdmmEnsemble(w.cost, homes, w.load, w.node_of, w.Rn, _kernels=k, **kw), (n * S, T), (n, S * T))
    recorded(lambda k: AdmmEngine(w.cost, homes[0], w.load, w.node_of, w.Rn, _kernels=k, **kw), (n, T), (n, T))


@pytest.mark.parametrize("S", [10, 12])
def test_a_newton_failure_beyond_the_admm_forms_columns_is_a_named_error(S):
    """240 and 288 columns (S = 10, 12 at T = 24), the Newton path made to give up (newton_max = 0) once rows bind: the
    ADMM forms hold 192 columns in an ensemble (their dense products), so the iteration ends in a RevsError that names
    scenario, slot and column -- never in an estimate (P_est_new stays what the failed evaluation left, P_est untouched)."""
    from fake_kernels import FakeKernels
    from helpers import f32
    from revs_admm_amd._lib import RevsError
    from revs_admm_amd.engine import OperatorOptions
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(150, 24, n_nodes=15, seed=11, binary_feasible=False, stress=1.5)
    w.load, w.cost = f32(w.load), f32(w.cost)
    e = AdmmEnsemble(w.cost, [w.homes] * S, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                     mode="relaxed_exact", device="cpu", op=OperatorOptions(newton_max=0), _kernels=FakeKernels())
    assert e.T == 24 * S
    e.step()                                     # (iteration 1: zero state, no row binds, no Newton iteration needed)
    before, it = e.P_est.clone(), e.iteration
    with pytest.raises(RevsError, match=r"scenario \d+, slot \d+ \(column \d+\).*192 columns"):
        e.step()
    assert e.iteration == it and (e.P_est == before).all() and e.op_path_hist == ["dual"]


def test_rounding_the_state_to_float_moves_exact_ties_of_the_golden_feeder(golden, feeder_R):
    """Why tests/test_gpu_ensemble.py holds the on/off pattern of a teacher-forced step against the oracle's home solve of
    the SAME float state: on the 121144 feeder (90 % adoption, seed 1234) the oracle's home solve of its own state at
    iteration index 1, once that state is rounded to float, picks other slots than its next iterate for 97 of 1126
    residences (8.6 %: more than the 5 % test_binary_teacher_forced's bar leaves) -- exact ties, the two choices'
    objectives within 1e-12 of each other in the double state; at index 2 the two agree everywhere."""
    from helpers import f32
    from oracle import revs_oracle as ro
    from revs_admm_amd.engine import pack_homes
    z, _ = golden
    com = z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]
    idx = {int(h): i for i, h in enumerate(z["res_id"])}
    np.random.seed(1234)
    ev = np.zeros(len(idx), bool)
    ev[[idx[int(h)] for h in np.random.choice(com, int(0.9 * len(com)), replace=False)]] = True
    load, cost = f32(z["LOAD"]), f32(z["tariff_shift6"])
    n = len(load)
    oh = ro.homes_from_records(load, pack_homes(ev, 4.8, 20.0, 0.2, 11, 23))
    tr = ro.solve_ADMM(oh, feeder_R, np.arange(n), cost, 5.0, 3, 1.03, 0.95, 1.05, mode="binary", keep=True,
                       util_eps=1e-10)[-1]
    share = []
    for k in (1, 2):
        dbl = (tr.P_est[k - 1], tr.P_sch[k - 1], tr.G[k - 1])
        assert np.array_equal(ro.home_solve_binary(cost, oh, *dbl, 5.0)[0], tr.S[k])
        p_f = ro.home_solve_binary(cost, oh, *[f32(a) for a in dbl], 5.0)[0]
        differ = np.abs(p_f - tr.S[k]).max(axis=1) != 0
        share.append(1.0 - differ.mean())
        gap = ro.home_objective(cost, oh, p_f, *dbl, 5.0) - ro.home_objective(cost, oh, tr.S[k], *dbl, 5.0)
        assert np.abs(gap[differ]).max(initial=0.0) < 1e-12
        assert (p_f[differ].sum(axis=1) == tr.S[k][differ].sum(axis=1)).all()       # the same energy, other slots
    print("share of residences whose pattern survives the rounding, iteration index 1, 2:", share)
    assert share[0] < 0.95 and int(round((1 - share[0]) * n)) == 97 and share[1] == 1.0
