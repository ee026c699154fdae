"""AdmmEnsemble.lower_bounds / certificates and the call surface around them, on the host: the driver -- the (S, M, T)
multipliers into the operator's view, the column slices of the dense product past 192 columns, the per-scenario cost,
worst row and gap, the lock-step search -- over the numpy stand-in of the kernels (tests/fake_kernels.py) with
revs_dual_bound_many restated through tests/bound_ref.py.  The kernel itself is tests/test_gpu_bound_many.py's job."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def _fake():
    from bound_ref import dual_bound
    from fake_kernels import FakeKernels, view
    from revs_admm_amd._lib import HOME_DTYPE

    class FakeMany(FakeKernels):
        """+ revs_dual_bound_many on the ensemble's layout: records [n][S], columns s T + t of double[m][S T]."""
        launches = 0

        def revs_dual_bound_many_scratch(self, n, S, T):
            return 2 * S * (T + -(-n // 32))

        def revs_dual_bound_many(self, n, S, T, cost, homes, node_of, m, d, y, load_node, scale, vlo, vhi, integral,
                                 scratch, out, stream):
            type(self).launches += 1
            c = view(cost, (T,), np.float32)
            sc, o = view(scale, (S,), np.float64), view(out, (S, 4), np.float64)
            cols = lambda p: view(p, (m, S, T), np.float64) if p else None
            dd, yy, ll = cols(d), cols(y), cols(load_node)
            recs = view(homes, (n, S, 32), np.uint8) if n else None
            nodes = view(node_of, (n,), np.int32) if n else np.zeros(0, np.int32)
            for s in range(S):
                ys, ds = (yy[:, s], dd[:, s]) if yy is not None else (np.zeros((m, T)), np.zeros((m, T)))
                h = np.ascontiguousarray(recs[:, s]).view(HOME_DTYPE).reshape(n) if n else np.zeros(0, HOME_DTYPE)
                _, parts, empty, _, _ = dual_bound(c, h, np.zeros((n, T)), nodes, np.zeros((m, m)), ys, sc[s], vlo, vhi,
                                                   integral=bool(integral), d=ds)
                load = float(((c.astype(np.float64)[None, :] + sc[s] * ds) * ll[:, s]).sum()) if ll is not None else 0.0
                o[s] = parts["home"], load, parts["row"], empty
            return 0
    return FakeMany


def _scenarios(n, T, S, seed=5):
    """EV ownership, ratings and windows of each scenario's own (as test_ensemble_host.py draws them)."""
    from revs_admm_amd.engine import pack_homes
    rng = np.random.default_rng(seed)
    capacity, start, end = rng.choice([20.0, 40.0, 60.0], n), rng.integers(10, 14, n), rng.integers(21, 25, n)
    homes = []
    for s in range(S):
        rating = (3.6, 4.8, 7.2)[s % 3]
        ev = rng.random(n) < (0.3, 0.5, 0.7)[s % 3]
        initial = np.maximum(np.clip(0.9 - rng.uniform(0.3, 0.7, n), 0.05, 0.85),
                             0.9 - 0.9 * rating / capacity * (end - start - 1))
        homes.append(pack_homes(ev, rating, capacity, initial, start, end))
    return homes


@pytest.mark.parametrize("S", [3, 9])
def test_the_driver_on_the_host_stand_in(S):
    """72 columns (one dense product) and 216 (column slices of whole scenarios: 8 + 1): every scenario's bound, cost,
    worst row and gap against numpy on that scenario alone."""
    from bound_ref import dual_bound
    from helpers import f32
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.engine import voltage_limits
    from revs_admm_amd.synthetic import make_workload
    Fake = _fake()
    n, T = 150, 24
    w = make_workload(n, T, n_nodes=15, seed=11, binary_feasible=False, stress=1.0)
    w.load, w.cost = f32(w.load), f32(w.cost)
    rng = np.random.default_rng(S)
    homes = _scenarios(n, T, S)
    homes[1]["end"][np.flatnonzero(homes[1]["ev"])[:2]] = 0             # two residences with empty rows in scenario 1
    load = np.stack([w.load] * S)
    load[1] = f32(w.load * rng.uniform(0.8, 1.2, w.load.shape))
    e = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                     mode="relaxed_exact", device="cpu", _kernels=Fake())
    assert e.T == S * T
    P_sch = f32(load + rng.uniform(0.0, 2.0, load.shape) * (rng.random(load.shape) < 0.2))
    for s in range(S):
        e.set_state(s, P_sch[s], P_sch[s], np.zeros((n, T)))
    y = np.zeros((S, w.M, T))
    mask = rng.random(y.shape) < 0.08
    y[mask] = rng.choice([-1.0, 1.0], mask.sum()) * rng.uniform(0.05, 3.0, mask.sum())
    y[2] = 0.0                                                         # a scenario without multipliers
    scale = rng.uniform(0.0, 3.0, S)
    scale[0] = 0.0
    vlo, vhi = voltage_limits(w.vset, w.vlow, w.vhigh)
    ref = lambda s, x, integral=False: dual_bound(w.cost, homes[s], load[s], w.node_of, w.Rn, y[s], x, vlo, vhi,
                                                  integral=integral)
    for integral in (False, True):
        got = e.lower_bounds(y, scale, integral=integral)
        assert got.shape == (S,) and got.dtype == np.float64
        for s in range(S):
            val, _, empty, _, _ = ref(s, scale[s], integral)       # (on/off chargers: some records reach no level in 0.9..1)
            assert empty >= 2 if s == 1 else integral or not empty
            assert math.isinf(got[s]) if empty else abs(got[s] - val) <= 1e-12 * abs(val), (s, got[s], val, empty)
    one = e.lower_bounds(y, 1.0)
    assert all(abs(one[s] - ref(s, 1.0)[0]) <= 1e-12 * abs(ref(s, 1.0)[0]) for s in range(S) if s != 1)
    assert np.array_equal(e.lower_bounds(), e.lower_bounds(np.zeros_like(y), 0.0))      # (no solve yet: no support)
    with pytest.raises(ValueError, match="scale"):
        e.lower_bounds(y, -1.0)
    with pytest.raises(ValueError, match="scale"):
        e.lower_bounds(y, np.ones(S + 1))
    with pytest.raises(ValueError, match="scale"):
        e.lower_bounds(y, np.full(S, np.nan))
    with pytest.raises(ValueError, match="multipliers"):
        e.lower_bounds(y[0])
    # ---- certificates at s = 1
    state = [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)]
    Fake.launches = 0
    certs = e.certificates(multipliers=y, search=False)
    assert Fake.launches == 3 and len(certs) == S                      # c.P_sch, c.LOAD, one evaluation
    for s, c in enumerate(certs):
        upper = float((w.cost[None, :] * P_sch[s]).sum())
        lsum = np.zeros((w.M, T))
        np.add.at(lsum, w.node_of, P_sch[s])
        v = w.Rn @ lsum
        viol = max(0.0, (v - vhi).max(), (vlo - v).max())
        assert abs(c.upper - upper) <= 1e-12 * upper
        assert abs(c.max_violation - viol) <= 1e-12 * max(abs(vlo), abs(vhi)) and c.feasible == (viol <= e.op.eps * e._scale)
        assert c.scale == (0.0 if s == 2 else 1.0) and c.evaluations == 1 and c.ascent_steps == 0 and not c.integral
        assert c.empty == (2 if s == 1 else 0) and c.seconds == certs[0].seconds
        if s == 1:
            assert math.isinf(c.lower) and math.isinf(c.gap) and math.isinf(c.gap_ev)
            continue
        val = ref(s, c.scale)[0]
        assert abs(c.lower - val) <= 1e-12 * abs(val)
        assert abs(c.gap - (c.upper - c.lower) / abs(c.lower)) <= 1e-15
        charge = c.lower - float((w.cost[None, :] * load[s]).sum())
        assert abs(c.gap_ev - (c.upper - c.lower) / abs(charge)) <= 1e-9 * abs(c.gap_ev)
    # ---- the search in lock-step
    searched = e.certificates(multipliers=y, search=True)
    l0 = e.lower_bounds(y, 0.0)
    for s, c in enumerate(searched):
        assert c.evaluations == searched[0].evaluations <= 2 + 60 + 48
        if s == 1:
            assert math.isinf(c.lower) and c.scale == 0.0
            continue
        assert c.lower >= max(l0[s], one[s]) and c.upper == certs[s].upper
        val = ref(s, c.scale)[0]
        assert abs(c.lower - val) <= 1e-12 * abs(val)
    assert searched[2].scale == 0.0 and searched[2].lower == l0[2]
    for a, b in zip(state, (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_the_singular_methods_name_the_plural_ones():
    from revs_admm_amd.ensemble import AdmmEnsemble
    for name in ("lower_bound", "certificate", "network_report", "voltage"):
        with pytest.raises(NotImplementedError, match=r"lower_bounds\(\) / certificates\(\)"):
            getattr(AdmmEnsemble, name)(None)


def test_study_certify_needs_and_uses_the_ensemble(golden, monkeypatch):
    """REVS.study(certify=True): refused without ensemble=True; with it, solve_ADMM_many is asked for the certificates
    and labels[s]["certificate"] holds each distributed scenario's, in grid order; the default leaves labels as they are."""
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
    asked = []

    def many(homes_list, graph, cost, grbpath=None, return_certificates=False, **kw):
        asked.append(return_certificates)
        sols = [(None, {h: homes[h]["LOAD"] for h in res}, None, None) for homes in homes_list]
        return (sols, [f"certificate {i}" for i in range(len(sols))]) if return_certificates else sols

    monkeypatch.setattr(revs_fixture, "solve_ADMM_many", many)
    monkeypatch.setattr(REVS, "get_individual_optimal",
                        lambda self, tariff, homes, save=False, **kw: ({h: homes[h]["LOAD"] for h in res}, None, None))
    fx = REVS(device="cpu")
    grid = dict(adoptions=(30, 90), ratings=(4800,), seeds=(1234,), max_iterations=3)
    with pytest.raises(ValueError, match="ensemble=True"):
        fx.study(tariff, all_homes, dist, com, certify=True, **grid)
    assert asked == []
    lab0, _ = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)
    lab1, _ = fx.study(tariff, all_homes, dist, com, ensemble=True, certify=True, **grid)
    assert asked == [False, True]
    assert all("certificate" not in lab for lab in lab0)
    dis = [lab for lab in lab1 if lab["method"] == "distributed"]
    assert [lab["certificate"] for lab in dis] == ["certificate 0", "certificate 1"]
    assert all("certificate" not in lab for lab in lab1 if lab["method"] == "individual")
    assert [{k: v for k, v in lab.items() if k != "certificate"} for lab in lab1] == lab0


def test_no_scenarios_no_certificates():
    from revs_admm_amd.lpsolver import solve_ADMM_many
    import networkx as nx
    assert solve_ADMM_many([], nx.Graph(), [1.0] * 24) == []
    assert solve_ADMM_many([], nx.Graph(), [1.0] * 24, return_certificates=True) == ([], [])
