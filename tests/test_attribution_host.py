"""The attribution report's contract on the host (no GPU): the restatement of tests/attr_ref.py against the all-pairs
definition.

sens against the dense R.  headroom_ref.lca_matrix builds R[i][j] = wc[lca(i, j)] by a naive pairwise walk over the same
wc -- the same additions, parents first -- so the row R[j*] equals sens in BYTES; that is what is asserted on every shape.
network_ref.dense builds R from two explicit inverses and a matrix product, whose path sums are added in another order:
against it sens is held to 2^-52 relative, |sens - R[j*]| <= 2^-52 R[j*]; the worst figure is printed (0 on the forests of
13 and 300 nodes, 1.9e-16 on the one of 2056).

total against drop[j*]: |total - drop[j*]| <= BOUND x max|drop| with test_gpu_network.BOUND = 1e-12."""
import numpy as np
import pytest

import attr_ref as ar
import headroom_ref as hr
import network_ref as nr
from test_gpu_network import BOUND, golden_net, synthetic_forest  # noqa: F401  (golden_net: a fixture)

from revs_admm_amd.feeder import feeder_tree, headroom_aux, tree_report_host


def setup(parent, edge_r, cons_of, p, ev=None, limit=None):
    """-> dict(tree, aux, n, inj, ev, drop, limit) by preorder position (the scans restated by tree_report_host)."""
    parent = np.asarray(parent, np.int64)
    n = len(parent)
    tree = feeder_tree(parent, edge_r, cons_of, np.ones(p.shape[0], bool))
    aux = headroom_aux(tree)
    _, drop = tree_report_host(tree, p, n)
    rows = lambda a: np.where((tree["src"] >= 0)[:, None], a[np.maximum(tree["src"], 0)], 0.0)
    lim = None if limit is None else hr.to_pos(tree, np.asarray(limit, bool), False)
    return dict(tree=tree, aux=aux, n=n, inj=rows(p), ev=None if ev is None else rows(ev), drop=hr.to_pos(tree, drop),
                limit=lim)


def run(c, drop_max, frac=0.01, **kw):
    return ar.contract(c["tree"], c["aux"], c["n"], c["inj"], c["ev"], c["drop"], drop_max, frac, limit=c["limit"], **kw)


def watched_positions(c, out):
    order = c["tree"]["order"]
    pos = np.full(c["tree"]["n"] + 1, -1)
    pos[order] = np.arange(c["tree"]["n"])
    return [int(pos[w]) if w >= 0 else -1 for w in out["slot"]["watch"]]


def random_forest(n, rng, zero=0.15):
    parent = np.full(n, -1, np.int64)
    for i in range(1, n):
        parent[i] = rng.integers(max(0, i - 40), i) if rng.random() < 0.93 else -1
    er = rng.uniform(0.5, 1.5, n)
    er[rng.random(n) < zero] = 0.0                              # zero-weight edges
    return parent, er


@pytest.mark.parametrize("n", [13, 300, 2056])
def test_sens_is_the_dense_row_and_total_is_the_drop(n):
    rng = np.random.default_rng(n)
    parent, er = random_forest(n, rng)
    rows = np.flatnonzero(rng.random(n) < 0.7)
    cons = np.full(n, -1, np.int64)
    cons[rows] = np.arange(len(rows))
    p = rng.uniform(0.0, 1.0, (len(rows), 3))
    ev = p * rng.uniform(0.0, 1.0, p.shape)
    c = setup(parent, er, cons, p, ev, rng.random(n) < 0.6)
    dmax = float(np.quantile(c["drop"], 0.9))
    out = run(c, dmax)
    aux = c["aux"]
    R = hr.lca_matrix(aux["parent_pos"], aux["depth"], aux["wc"]) if n <= 300 else None
    eu = np.where(parent < 0, n, parent)
    Rd = nr.dense(n + 1, eu, np.arange(n), er, np.arange(n))[1]
    depth = int(aux["depth"].max()) + 1
    worst = 0.0
    for t, j in enumerate(watched_positions(c, out)):
        assert j >= 0
        if R is not None:
            assert out["sens"][:, t].tobytes() == R[j].tobytes()                  # the same additions: bytes
        else:                                                                      # (2056: the walk of one row)
            row = hr.lca_matrix(aux["parent_pos"], aux["depth"], aux["wc"])[j] if t == 0 else None
            assert row is None or out["sens"][:, t].tobytes() == row.tobytes()
        order = c["tree"]["order"]
        real = order < n
        dense_row = Rd[order[j]][order[real]]
        got = out["sens"][real, t]
        err = np.abs(got - dense_row)
        assert (err <= 2.0 ** -52 * np.abs(dense_row)).all()
        worst = max(worst, float((err / np.maximum(np.abs(dense_row), 1e-300)).max()))
        gap = abs(out["slot"]["total"][t] - c["drop"][j, t])
        assert gap <= BOUND * np.abs(c["drop"]).max(), (gap, np.abs(c["drop"]).max())
        assert out["slot"]["drop_watch"][t] == c["drop"][j, t]
        assert abs(out["slot"]["ev_total"][t]) <= abs(out["slot"]["total"][t])
    print(f"forest of {n}: sens against the inverse-based dense R, worst relative error {worst:.3e} (depth {depth})")


def chain(n, r=1.0):
    return np.arange(-1, n - 1), np.full(n, r), np.arange(n)


def test_hand_cases():
    # a chain of 8, every node a limit node: the last one is watched, sens = wc
    c = setup(*chain(8, 0.5), np.ones((8, 1)) / 64)
    out = run(c, 0.1)
    assert watched_positions(c, out) == [7] and out["sens"][:, 0].tobytes() == c["aux"]["wc"].tobytes()
    assert out["slot"]["n_reach"][0] == 8
    # a star: only the watched leaf reaches itself
    c = setup(np.full(6, -1), np.ones(6), np.arange(6), np.arange(1.0, 7.0)[:, None] / 32)
    out = run(c, 0.1)
    assert watched_positions(c, out) == [5] and out["slot"]["n_reach"][0] == 1
    assert np.array_equal(out["sens"][:, 0] > 0, np.arange(8) == 5)
    # two roots plus padding (5 nodes pad to 8): the other tree's sens is +0.0, padding too
    c = setup(np.array([-1, 0, 0, -1, 3]), np.ones(5), np.arange(5), np.array([[1.0], [1.0], [1.0], [1.0], [3.0]]) / 64)
    out = run(c, 0.05)
    order = c["tree"]["order"]
    assert out["slot"]["watch"][0] == 4
    other = np.isin(order, [0, 1, 2]) | (order >= 5)
    assert out["sens"][other, 0].tobytes() == np.zeros(int(other.sum())).tobytes()
    assert (out["sens"][np.isin(order, [3, 4]), 0] > 0).all() and out["slot"]["n_reach"][0] == 2
    # a tie of two limit nodes on drop: the lowest caller-side index wins
    c = setup(np.array([-1, 0, 0]), np.array([1.0, 0.5, 0.5]), np.arange(3), np.array([[0.0], [0.25], [0.25]]))
    assert c["drop"][1, 0] == c["drop"][2, 0] > c["drop"][0, 0]
    assert run(c, 0.1)["slot"]["watch"][0] == 1
    # a fixed watch
    pos0 = int(np.flatnonzero(c["tree"]["order"] == 0)[0])
    out = run(c, 0.1, watch_pos=pos0)
    assert out["slot"]["watch"][0] == 0 and (out["sens"][:3, 0] == c["aux"]["wc"][pos0]).all()
    # no limit node at all: no candidate, everything +0.0
    c["limit"] = np.zeros(c["tree"]["n"], bool)
    out = run(c, 0.1)
    assert out["slot"]["watch"][0] == -1 and not out["sens"].any() and out["summary"][0]["count"] == 0
    assert out["slot"]["n_reach"][0] == 0 and out["contrib"].tobytes() == np.zeros_like(out["contrib"]).tobytes()


def test_excess_zero_and_relief_equal_to_ev():
    # chain of 4, r = 0.5 (w = 1, wc = 1, 2, 3, 4), load 1 at the end: drop = 1, 2, 3, 4
    par, er, cons = chain(4, 0.5)
    p = np.array([[0.0], [0.0], [0.0], [1.0]])
    c = setup(par, er, cons, p, ev=p)
    out = run(c, 8.0)                                            # no excess: every relief 0, n_can 0
    assert out["slot"]["excess"][0] == 0.0 and out["slot"]["n_can"][0] == 0
    assert not ar.relief(out["sens"], out["slot"]["excess"]).any()
    # drop_max = 2: excess = 2; relief = 2 / wc = 2, 1, 2/3, 0.5; ev exactly 0.5 at the last node counts, and no other
    ev = np.array([[1.0], [0.5], [0.5], [0.5]])
    c = setup(par, er, cons, p, ev=ev)
    out = run(c, 2.0)
    rel = ar.relief(out["sens"], out["slot"]["excess"])
    assert out["slot"]["excess"][0] == 2.0 and rel[3, 0] == 0.5 == c["ev"][3, 0]
    assert out["slot"]["n_can"][0] == 1 and out["slot"]["n_reach"][0] == 4
    ev[3, 0] = np.nextafter(0.5, 0.0)                            # one ulp short: no longer
    c = setup(par, er, cons, p, ev=ev)
    assert run(c, 2.0)["slot"]["n_can"][0] == 0
    # a node that shares no edge with the watched one: relief +inf
    c = setup(np.array([-1, -1]), np.ones(2), np.arange(2), np.array([[0.0], [1.0]]))
    out = run(c, 0.5)
    assert np.isinf(ar.relief(out["sens"], out["slot"]["excess"])[0, 0])


def test_bad_slot_and_counts():
    rng = np.random.default_rng(3)
    parent, er = random_forest(60, rng, zero=0.0)
    p = rng.uniform(0.0, 1.0, (60, 3))
    ev = 0.5 * p
    ev[7, 1] = np.inf
    c = setup(parent, er, np.arange(60), p, ev)
    out = run(c, float(np.quantile(c["drop"], 0.5)), cls=np.arange(c["tree"]["n"]) % 3, C=3)
    assert out["slot"]["n_bad"].tolist() == [0, 1, 0] and out["slot"]["watch"][1] == -1
    assert np.isnan(out["sens"][:, 1]).all() and np.isnan(out["slot"]["class_total"][1]).all()
    assert out["summary"][1]["count"] == 0 and out["summary"][1]["n_nan"] == 60
    for t in (0, 2):
        s = out["slot"]
        assert s["n_reach"][t] == out["summary"][t]["count"] >= s["n_big"][t] >= 1
        assert s["top_value"][t, 0] == out["summary"][t]["worst_value"] and s["top_index"][t, 0] == out["summary"][t]["worst_index"]
        assert (np.diff(s["top_value"][t][~np.isnan(s["top_value"][t])]) <= 0).all()
        assert abs(s["class_total"][t, :3].sum() - s["total"][t]) <= 1e-12 * abs(s["total"][t])
    assert (out["day"]["peak_slot"] != 1).all()


@pytest.fixture(scope="module")
def golden_runs(golden, golden_net):
    """The stored 121144 results under both schedules: contract() with the EV part = P_res - LOAD, and the dense R."""
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    load = np.asarray(z["LOAD"], np.float64)
    runs = {}
    for tag in ("dis_a90_r4800", "ind_a90_r4800"):
        p = np.asarray(z[tag + "_P_res"], np.float64)
        c = setup(par, er, cons, p, p - load)
        runs[tag] = (c, run(c, 1.0 - 0.95 ** 2))
    return runs


def test_stored_results_of_the_reference(golden_runs, golden_net):
    gn = golden_net
    dmax = 1.0 - 0.95 ** 2
    share = {}
    for tag, (c, out) in golden_runs.items():
        order, s = c["tree"]["order"], out["slot"]
        real = order < gn["n"]
        P = np.zeros((gn["n"], 24))
        P[order[real]] = c["inj"][real]
        EV = np.zeros((gn["n"], 24))
        EV[order[real]] = c["ev"][real]
        RP = gn["R"] @ P
        for t in (14, 15, 16, 20):                               # everything from the dense form
            w = int(s["watch"][t])
            assert w == int(gn["rows"][np.argmax(RP[gn["rows"], t])]) or \
                abs(RP[w, t] - RP[gn["rows"], t].max()) <= BOUND * np.abs(RP).max()
            total_d, ev_d = gn["R"][w] @ P[:, t], gn["R"][w] @ EV[:, t]
            assert abs(s["total"][t] - total_d) <= BOUND * np.abs(RP).max()
            assert abs(s["ev_total"][t] - ev_d) <= BOUND * np.abs(RP).max()
            assert abs(s["total"][t] - s["drop_watch"][t]) <= BOUND * np.abs(c["drop"]).max()
            if t != 20:
                assert RP[w, t] > dmax and s["excess"][t] > 0.0                  # the worst node is violated ...
                assert abs(ev_d) <= 1e-12 * total_d and abs(s["ev_total"][t]) <= 1e-12 * s["total"][t]   # ... by the base load alone
            row = gn["R"][w]                                     # (an inverse-based R: its zeros are zeros within rounding)
            assert s["n_reach"][t] < c["tree"]["n"] and s["n_reach"][t] == int((row > 1e-9 * row.max()).sum())
        share[tag] = (gn["R"][int(s["watch"][20])] @ EV[:, 20]) / (gn["R"][int(s["watch"][20])] @ P[:, 20])
        assert abs(share[tag] - s["ev_total"][20] / s["total"][20]) <= 1e-9
    print("EV share of the worst node's drop in slot 20:", share)
    assert 0.5 < share["dis_a90_r4800"] < share["ind_a90_r4800"] < 0.9
