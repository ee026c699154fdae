"""AdmmEnsemble.node_sums / study_report / network_reports and the call surface above them (revs_admm_amd/
ensemble_report.py, DESIGN.md section 3.9 "Reports") on the GPU: the node sums are the sequential float64 sums of the
schedules the ensemble returns, exactly; every field of the report is, bit for bit, what the host-upload entries
(study.study_report, network.report_for_tree) give when fed the same node sums; the run's state is left alone;
solve_ADMM_many(return_node_sums=True) and REVS.study(device_report=True) hand the same numbers on without a read-back."""
import numpy as np
import pytest

from network_worker import line_ratings
from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
from test_gpu_network import _lines
from test_gpu_study import BANDS, same_study

pytestmark = pytest.mark.gpu


def _sequential_sums(e, prof64):
    """prof64 (S, n, T) float64 in the caller's residence order -> (S, M, T): one accumulator per output, the
    residences in the engine's order (e.perm: ascending node, then ascending index)."""
    out = np.zeros((prof64.shape[0], e.M, prof64.shape[2]))
    node_of = np.repeat(np.arange(e.M), np.asarray(e.node_counts))
    for k, i in enumerate(e.perm):
        out[:, node_of[k], :] = out[:, node_of[k], :] + prof64[:, i, :]
    return out


def _same_report(a, b, arrays):
    assert same_study(a, b)
    assert a.groups.tolist() == b.groups.tolist() and a.bands == b.bands
    assert (a.vset, a.vmin, a.vmax) == (b.vset, b.vmin, b.vmax)
    assert a.node_p.tobytes() == b.node_p.tobytes()
    for k in ("flow", "loading", "volt"):
        if arrays:
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
        else:
            assert getattr(a, k) is None and getattr(b, k) is None


def _mixed_ensemble(iters):
    """600 residences on 60 nodes, T = 24, five mixed scenarios, scenario 3's load perturbed (test_gpu_ensemble's)."""
    from helpers import f32
    w = _workload()
    homes = _mixed_scenarios(w, 5)
    load = np.stack([w.load] * 5)
    load[3] = f32(w.load * np.where(w.node_of < 20, 1.5, 0.9)[:, None]
                  * np.random.default_rng(2).uniform(0.95, 1.05, w.load.shape))
    e = _ensemble(w, homes, "relaxed_exact", load=load)
    e.run(iters)
    return w, load, e


def test_synthetic_ensemble_report(gpu_lib):
    from revs_admm_amd import study
    from revs_admm_amd.network import report_for_tree
    w, load, e = _mixed_ensemble(3)
    assert (np.asarray(e.node_counts) > 0).all()                 # every node has a residence
    rating, nodes = line_ratings(w)
    par, er, cons = w.feeder
    groups = [0, 0, 1, 1, -1]
    rep = e.study_report(groups=groups, rating=rating, nodes=nodes, arrays=True)
    P, Sp, _ = e.result()
    # a. the node sums: sequential float64 sums of the schedules in the engine's residence order, exactly
    assert rep.node_p.shape == (5, w.M, 24) and rep.node_p.dtype == np.float64
    assert rep.node_p.tobytes() == _sequential_sums(e, P.astype(np.float64)).tobytes()
    assert np.abs(rep.node_p[3] - rep.node_p[0]).max() > 0.1     # (no broadcast of one scenario)
    # b. every field: the host-upload entry fed the same bytes
    ref = study.study_report(par, er, cons, rep.node_p, groups=groups, rating=rating, nodes=nodes, bands=BANDS,
                             vset=w.vset, vmin=w.vlow, vmax=w.vhigh, arrays=True)
    _same_report(rep, ref, arrays=True)
    assert rep.n_groups == 2 and rep.band_counts.shape == (5, 24, 3) and rep.volt.shape == (5, len(par), 24)
    assert (rep.pooled_volt["count"] == 2 * len(nodes)).all()
    # c. the per-scenario reports from the same launch
    reports = e.network_reports(rating=rating, nodes=nodes)
    assert len(reports) == 5
    for s, r in enumerate(reports):
        one = report_for_tree(par, er, cons, rep.node_p[s], rating=rating, nodes=nodes, vset=w.vset, vmin=w.vlow,
                              vmax=w.vhigh)
        for k in ("flow", "loading", "volt", "node_sums", "summary_loading", "summary_volt"):
            assert getattr(r, k).tobytes() == getattr(one, k).tobytes(), (s, k)
        assert (r.vset, r.vmin, r.vmax) == (one.vset, one.vmin, one.vmax)
        assert r.worst_node == one.worst_node and r.worst_line == one.worst_line
    # d. an EV-only profile in the caller's order, the engine's load added on the device
    g = e.node_sums(profile=Sp, add_load=True).cpu().numpy()
    assert g.tobytes() == _sequential_sums(e, load.astype(np.float64) + Sp.astype(np.float64)).tobytes()
    assert np.abs(g - rep.node_p).max() < 1e-3                   # (P_sch IS load + S, to float rounding)
    # ... and the same profile as a device tensor in the engine's layout
    gd = e.node_sums(profile=e.S, add_load=True).cpu().numpy()
    assert gd.tobytes() == g.tobytes()


def test_reports_leave_the_state_alone(gpu_lib):
    w = _workload()
    homes = _mixed_scenarios(w, 5)
    rating, nodes = line_ratings(w)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for e in (a, b):
        e.run_steps(3)
    b.study_report(groups=[0, 0, 1, 1, -1], rating=rating, nodes=nodes, arrays=True)
    for k in range(3):
        a.step()
        b.step()
        if k == 0:
            b.network_reports(rating=rating, nodes=nodes)
        if k == 1:
            b.node_sums(add_load=True)
            b.study_report(rating=rating)
    assert a.iteration == b.iteration == 6
    for s in range(5):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
        assert a.multipliers(s).tobytes() == b.multipliers(s).tobytes(), s
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()


def test_wide_ensemble_report(gpu_lib):
    """3 scenarios at T = 96: 288 columns, beyond anything revs_net_node_sums takes."""
    from revs_admm_amd import study
    w = _workload(300, 96, 40, 17, stress=1.3)
    e = _ensemble(w, _mixed_scenarios(w, 3), "relaxed_exact")
    assert e.T == 288
    e.run(2)
    rating, nodes = line_ratings(w)
    par, er, cons = w.feeder
    rep = e.study_report(groups=[0, 1, 0], rating=rating, nodes=nodes, arrays=False)
    P = e.result()[0]
    assert rep.node_p.tobytes() == _sequential_sums(e, P.astype(np.float64)).tobytes()
    ref = study.study_report(par, er, cons, rep.node_p, groups=[0, 1, 0], rating=rating, nodes=nodes, bands=BANDS,
                             vset=w.vset, vmin=w.vlow, vmax=w.vhigh, arrays=False)
    _same_report(rep, ref, arrays=False)


# ---------------------------------------------------------------------------------------------------------------
# the call surface
# ---------------------------------------------------------------------------------------------------------------
def _dict_rows(sol, res):
    return np.array([sol[1][h] for h in res], np.float64)


def test_solve_many_returns_the_node_sums(gpu_lib, golden):
    """The three scenarios of test_reference_call_surface_for_many on the 121144 feeder: one residence per row, so the
    tensor is float64 of the returned P_sch dicts."""
    import torch
    from test_gpu_ensemble import _nx_graph
    from revs_admm_amd.extract import get_homes_ev_param
    from revs_admm_amd.lpsolver import solve_ADMM_many
    z, fd = golden
    g = _nx_graph(fd, z)
    res = z["res_id"].tolist()
    all_homes = {h: z["LOAD"][i].tolist() for i, h in enumerate(res)}
    ev = z["dis_a90_r4800_ev_homes"]
    com = z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]
    np.random.seed(56)
    other = np.random.choice(com, int(0.3 * len(com)), replace=False)
    scen = [get_homes_ev_param(all_homes, g, other, 3.6, 20, 0.2, 11, 23),
            get_homes_ev_param(all_homes, g, ev, 4.8, 20, 0.2, 11, 23),
            get_homes_ev_param(all_homes, g, other, 7.2, 20, 0.2, 11, 23)]
    out, node_g = solve_ADMM_many(scen, g, z["tariff_shift6"].tolist(), "./gurobi", kappa=5.0, iter_max=2, vset=1.03,
                                  vlow=0.95, vhigh=1.05, return_node_sums=True)
    assert isinstance(node_g, torch.Tensor) and node_g.is_cuda and node_g.dtype == torch.float64
    assert tuple(node_g.shape) == (3, 1126, 24) and len(out) == 3
    got = node_g.cpu().numpy()
    for s in range(3):
        assert got[s].tobytes() == _dict_rows(out[s], res).tobytes(), s
    empty = solve_ADMM_many([], g, z["tariff_shift6"].tolist(), return_node_sums=True)
    assert empty[0] == [] and tuple(empty[1].shape) == (0, 1126, 24) and empty[1].dtype == torch.float64
    e3 = solve_ADMM_many([], g, z["tariff_shift6"].tolist(), return_certificates=True, return_node_sums=True)
    assert e3[:2] == ([], []) and tuple(e3[2].shape) == (0, 1126, 24)


def _small_graph(n_road=8, per=5):
    """A radial feeder of n_road x per residences: substation - transformer - road nodes in a chain, residences on each
    (node attribute 'label', edge attribute 'r', as test_network_host.golden_graph builds the golden one)."""
    import networkx as nx
    g = nx.Graph()
    g.add_node(0, label="S")
    g.add_node(1, label="T")
    g.add_edge(0, 1, r=2e-4)
    prev, nid = 1, 2
    for k in range(n_road):
        road = nid
        g.add_node(road, label="R")
        g.add_edge(prev, road, r=1e-4 * (1 + k % 3))
        nid += 1
        for _ in range(per):
            g.add_node(nid, label="H")
            g.add_edge(road, nid, r=3e-4)
            nid += 1
        prev = road
    return g


def test_several_ensembles_fill_one_buffer_in_order(gpu_lib):
    """Six scenarios at T = 192 hold five per ensemble: split_scenarios gives 3 + 3, each ensemble fills its slice."""
    from revs_admm_amd.extract import get_homes_ev_param
    from revs_admm_amd.lpsolver import solve_ADMM_many, split_scenarios
    T = 192
    assert split_scenarios(6, T) == [(0, 3), (3, 6)]
    g = _small_graph()
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    assert len(res) == 40
    rng = np.random.default_rng(4)
    base = {h: rng.uniform(0.2, 1.5, T).astype(np.float32).astype(np.float64).tolist() for h in res}
    tariff = (0.1 + 0.05 * np.sin(np.arange(T) / T * 2 * np.pi)).astype(np.float32).astype(np.float64).tolist()
    scen = []
    for s in range(6):
        evs = rng.choice(res, 8 + 4 * s, replace=False)
        loads = base if s != 4 else {h: (np.float32(1.25) * np.asarray(v, np.float32)).astype(np.float64).tolist()
                                     for h, v in base.items()}        # (one ensemble with loads of its scenarios' own)
        scen.append(get_homes_ev_param(loads, g, evs, (3.6, 4.8, 7.2)[s % 3], 160.0, 0.2, 88, 184))
    out, node_g = solve_ADMM_many(scen, g, tariff, None, kappa=5.0, iter_max=2, vset=1.03, vlow=0.95, vhigh=1.05,
                                  mode="relaxed", return_node_sums=True)
    assert tuple(node_g.shape) == (6, 40, T) and len(out) == 6
    got = node_g.cpu().numpy()
    rows = [_dict_rows(sol, res) for sol in out]
    for s in range(6):
        assert got[s].tobytes() == rows[s].tobytes(), s
        charged = np.array([sum(out[s][2][h]) for h in res])
        assert ((charged > 1.0) == np.array([scen[s][h]["EV"] != {} for h in res])).all(), s
    assert all(np.abs(rows[a] - rows[b]).max() > 0.1 for a in range(6) for b in range(a + 1, 6))


def test_study_device_report(gpu_lib, golden):
    """REVS.study(ensemble=True, device_report=True) on the grid of test_study_with_an_ensemble_equals_the_study_without:
    its report is study.study_report fed its own node_p; labels as without device_report; the node sums within that
    test's 4e-5 kW of the run that reads the schedules back (whether they are identical is printed)."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd import study
    from revs_admm_amd.drawing import line_nodes
    from revs_admm_amd.lpsolver import feeder_of
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    ln = _lines()
    table = {s.decode(): float(r) for s, r in zip(ln["type_name"], ln["type_rating"])}
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    grid = dict(adoptions=(30, 90), ratings=(4800,), seeds=(1234, 56), group_by=("method", "adoption"), max_iterations=15,
                v0=1.03, line_rating=table, arrays=True, mode="relaxed")
    with pytest.raises(ValueError, match="ensemble=True"):
        fx.study(tariff, all_homes, dist, com, device_report=True, **grid)
    lab0, rep0 = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)
    lab1, rep1 = fx.study(tariff, all_homes, dist, com, ensemble=True, device_report=True, **grid)
    assert lab1 == lab0 and rep1.groups.tolist() == rep0.groups.tolist()
    assert rep1.node_p.shape == rep0.node_p.shape == (8, 1126, 24)
    dp = float(np.abs(rep1.node_p - rep0.node_p).max())
    print(f"node sums with device_report against the schedules read back: largest difference {dp:.3e} kW "
          f"({'identical' if dp == 0.0 else 'not identical'})")
    assert dp <= 4e-5
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    par, er, cons = feeder_of(dist)[1]
    node_rating = line_nodes(dist, table, par, nonsub)[0]
    nodes = [nonsub.index(h) for h in com]
    ref = study.study_report(par, er, cons, rep1.node_p, groups=rep1.groups, rating=node_rating, nodes=nodes, bands=BANDS,
                             vset=1.0, vmin=0.95, vmax=1.05, arrays=True)
    _same_report(rep1, ref, arrays=True)
