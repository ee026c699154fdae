"""The network report on the host: the dense yard-stick (tests/network_ref.py) against the stored feeder, the numpy tree
restatement (feeder.tree_report_host) against the dense form at every node and line, and the argument handling of the
reference's call surface (drawing.compute_flows / compute_voltage, REVS.result_frames).  No GPU."""
import os

import numpy as np
import pytest

import network_ref as nr

HERE = os.path.dirname(os.path.abspath(__file__))
LINES = os.path.join(HERE, "golden", "revs_121144_lines.npz")


def golden_graph(golden, lines=True):
    import networkx as nx
    z, fd = golden
    ln = np.load(LINES)
    g = nx.Graph()
    for nid, lab in zip(z["node_id"], fd.label):
        g.add_node(int(nid), label=lab.decode())
    for k, (u, v, r) in enumerate(zip(fd.edge_u, fd.edge_v, fd.edge_r)):
        kw = dict(type=ln["edge_type"][k].decode()) if lines else {}
        g.add_edge(int(z["node_id"][u]), int(z["node_id"][v]), r=float(r), **kw)
    return g


def golden_tree(golden):
    """-> (graph, residences, non-substation nodes, feeder arrays, child tree node and sign of every edge)"""
    from revs_admm_amd.lpsolver import feeder_arrays
    z, fd = golden
    g = golden_graph(golden)
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    nonsub = [n for n in g if g.nodes[n]["label"] != "S"]
    par, er, cons = feeder_arrays(g, res)
    pos = {n: i for i, n in enumerate(nonsub)}
    child, sign = [], []
    for u, v in g.edges:
        down = v in pos and par[pos[v]] == pos.get(u, -1)
        child.append(pos[v] if down else pos[u])
        sign.append(1.0 if down else -1.0)
    return g, res, nonsub, (par, er, cons), np.array(child), np.array(sign)


def test_line_fixture_is_names_and_numbers():
    ln = np.load(LINES)
    assert os.path.getsize(LINES) < 16384
    assert len(ln["edge_type"]) == len(ln["edge_rating"]) == 1691
    counts = dict(zip((s.decode() for s in ln["type_name"]), ln["type_count"].tolist()))
    assert counts == {"OH_Voluta": 886, "OH_Swanate": 545, "OH_Periwinkle": 79, "OH_Conch": 67, "OH_Neritina": 39,
                      "OH_Zuzara": 36, "OH_Runcina": 19, "OH_Raven": 12, "OH_Penguin": 5, "OH_Sparrow": 3}
    np.testing.assert_allclose(ln["type_rating"], np.sqrt(3.0) * ln["type_ampacity"] * ln["type_kv"], rtol=1e-15)
    by = dict(zip(ln["type_name"], ln["type_rating"]))
    assert np.array_equal(ln["edge_rating"], [by[s] for s in ln["edge_type"]])


def test_dense_reference_reproduces_the_stored_feeder(golden, feeder_R):
    """network_ref's 2 F D F^T, restricted to the residences, is the matrix the existing fixtures give."""
    z, fd = golden
    nonsub, res = fd.nonsub(), fd.res()
    A_inv, R = nr.dense(fd.n_nodes, fd.edge_u, fd.edge_v, fd.edge_r, nonsub)
    pos = -np.ones(fd.n_nodes, np.int64)
    pos[nonsub] = np.arange(len(nonsub))
    ri = pos[res]
    assert np.abs(R[np.ix_(ri, ri)] - feeder_R).max() <= 1e-12 * np.abs(feeder_R).max()
    assert np.abs(R - R.T).max() <= 1e-12 * np.abs(R).max()


def test_tree_restatement_equals_dense_form_at_every_node_and_line(golden):
    """feeder.tree_report_host (the kernel's scans in numpy, every position kept) == F = A^-1 P at every line and
    R P at every non-substation node -- 1e-12 x the largest entry, the bound test_tree_voltage_matches_dense_product
    holds these sums to."""
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    z, fd = golden
    g, res, nonsub, (par, er, cons), child, sign = golden_tree(golden)
    A_inv, R = nr.dense(fd.n_nodes, fd.edge_u, fd.edge_v, fd.edge_r, fd.nonsub())
    tr = feeder_tree(par, er, cons, np.ones(len(res), bool))
    assert sorted(tr["order"].tolist()) == list(range(tr["n"])) and tr["n"] == 1696
    rng = np.random.default_rng(5)
    p = rng.uniform(0.0, 3.0, (len(res), 7))
    P = np.zeros((len(nonsub), 7))
    P[cons >= 0] = p[cons[cons >= 0]]
    flow, drop = tree_report_host(tr, p, len(par))
    F, RP = nr.flows(A_inv, P), R @ P
    assert np.abs(sign[:, None] * flow[child] - F).max() <= 1e-12 * np.abs(F).max()
    assert np.abs(drop - RP).max() <= 1e-12 * np.abs(RP).max()
    # (and at the residence rows it is tree_voltage_host)
    from revs_admm_amd.feeder import tree_voltage_host
    assert np.array_equal(tree_voltage_host(tr, p)[cons[cons >= 0]], drop[cons >= 0])


def test_box_stats_is_matplotlibs_rule():
    """network_ref.box_stats on a sample whose numbers are known by hand (and, where matplotlib is installed, equals it)."""
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 100.0, -50.0])
    b = nr.box_stats(x)
    assert (b["q1"], b["median"], b["q3"]) == (2.25, 4.5, 6.75)
    assert (b["whisker_lo"], b["whisker_hi"], b["n_fliers"], b["count"]) == (1.0, 8.0, 2, 10)
    assert nr.box_stats(np.array([3.0]))["whisker_hi"] == 3.0 and nr.box_stats(np.array([])) is None
    try:
        from matplotlib.cbook import boxplot_stats
    except ImportError:
        return
    m = boxplot_stats(x)[0]
    assert (m["q1"], m["med"], m["q3"], m["whislo"], m["whishi"], len(m["fliers"])) == \
        (b["q1"], b["median"], b["q3"], b["whisker_lo"], b["whisker_hi"], b["n_fliers"])


def test_compute_flows_needs_ratings(golden):
    from revs_admm_amd.drawing import compute_flows
    g = golden_graph(golden, lines=False)
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    p = {h: [0.0] * 24 for h in res}
    with pytest.raises(ValueError, match="needs line ratings"):
        compute_flows(g, p)
    g = golden_graph(golden)
    with pytest.raises(KeyError, match="OH_"):
        compute_flows(g, p, rating={"OH_Voluta": 39.5})
    e0 = next(iter(g.edges))
    g.edges[e0]["rating"] = 10.0                      # one edge rated is not every edge rated
    with pytest.raises(ValueError, match="needs line ratings"):
        compute_flows(g, p)


def test_reference_call_surface_keys_and_labels(golden, monkeypatch):
    """compute_flows / compute_voltage return the reference's dicts (edge tuples in graph.edges order, node ids of the
    non-substation nodes); result_frames the long tables of boxplot_flow / boxplot_volt with the reference's hour
    labels.  The report itself is replaced by the numpy tree restatement here (no GPU): the kernel is the GPU tests' job."""
    from revs_admm_amd import drawing, network
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    from revs_admm_amd.revs_fixture import REVS
    z, fd = golden
    ln = np.load(LINES)

    def host_report(parent, edge_r, cons_of, node_p, rating=None, nodes=None, vset=1.0, vmin=0.95, vmax=1.05,
                    arrays=True, device=None):
        tr = feeder_tree(parent, edge_r, cons_of, np.ones(len(node_p), bool))
        flow, drop = tree_report_host(tr, np.asarray(node_p, float), len(parent))
        rt = np.full(len(parent), np.nan) if rating is None else np.where(rating > 0, rating, np.nan)
        return network.NetworkReport(flow, np.abs(flow) / rt[:, None], np.sqrt(vset * vset - drop), None, None,
                                     node_p, vset, vmin, vmax)

    monkeypatch.setattr(drawing, "report_for_tree", host_report)
    g = golden_graph(golden)
    res = [n for n in g if g.nodes[n]["label"] == "H"]
    nonsub = [n for n in g if g.nodes[n]["label"] != "S"]
    demand = {h: z["dis_a90_r4800_P_res"][i].tolist() for i, h in enumerate(res)}
    table = {s.decode(): float(r) for s, r in zip(ln["type_name"], ln["type_rating"])}
    fl = drawing.compute_flows(g, demand, rating=table)
    assert list(fl) == list(g.edges) and all(len(v) == 24 for v in fl.values())
    vo = drawing.compute_voltage(g, demand, vset=1.0)
    assert list(vo) == nonsub and all(len(v) == 24 for v in vo.values())
    # the numbers are the dense formulas' (signs of the reference's edge orientation included)
    A_inv, R = nr.dense(fd.n_nodes, fd.edge_u, fd.edge_v, fd.edge_r, fd.nonsub())
    P = np.zeros((len(nonsub), 24))
    P[[nonsub.index(h) for h in res]] = z["dis_a90_r4800_P_res"]
    F = nr.flows(A_inv, P) / ln["edge_rating"][:, None]
    assert np.abs(np.array([fl[e] for e in g.edges]) - F).max() <= 1e-12 * np.abs(F).max()
    V = nr.volt(R, P, 1.0)
    assert np.abs(np.array([vo[n] for n in nonsub]) - V).max() <= 1e-12
    # per-edge `rating` attributes instead of the table
    for k, e in enumerate(g.edges):
        g.edges[e]["rating"] = float(ln["edge_rating"][k])
    assert drawing.compute_flows(g, demand) == fl
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    lf, vf = REVS(device="cpu").result_frames(demand, g, community=com, rating=table)
    assert lf["hour"].shape == lf["loading"].shape == (13 * 1691,)
    assert vf["hour"].shape == vf["voltage"].shape == (13 * len(com),)
    assert lf["hour"][0] == "16:00 - 17:00" and lf["hour"][-1] == "4:00 - 5:00"      # (t + shift - 1) % 24, t = 11..23
    assert vf["hour"][len(com)] == "17:00 - 18:00"
    np.testing.assert_allclose(lf["loading"][:1691], np.abs(F[:, 11]) * 100.0, rtol=0, atol=1e-10 * np.abs(F).max() * 100)
    np.testing.assert_allclose(vf["voltage"][:len(com)], V[[nonsub.index(h) for h in com], 11], rtol=0, atol=1e-12)


def test_network_report_without_a_tree_says_so():
    from fake_kernels import FakeKernels
    from revs_admm_amd.engine import AdmmEngine, OperatorOptions
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(200, 24, n_nodes=20, seed=1)
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="relaxed_exact", device="cpu", _kernels=FakeKernels(), op=OperatorOptions(voltage="dense"))
    assert e._tree is None
    with pytest.raises(ValueError, match="needs the feeder as a tree"):
        e.network_report()
