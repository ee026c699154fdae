"""The power-flow report's iteration on the host (no GPU): tests/powerflow_ref.py's solve() against the closed form of a
single line, against scipy.optimize.root handed the branch-flow equations whole on random trees, and on the 121144 feeder
under the stored distributed schedule -- passes, contraction factor, and the counts the report exists for, pinned."""
import os

import numpy as np
import pytest

import headroom_ref as hr
import powerflow_ref as pf

from revs_admm_amd.feeder import feeder_tree

HERE = os.path.dirname(os.path.abspath(__file__))
XFIX = os.path.join(HERE, "golden", "revs_121144_x.npz")


def positions(parent, edge_r, cons_of, p, edge_x=None):
    """-> (tree, inj by position, xw by position or None)."""
    tree = feeder_tree(parent, edge_r, cons_of, np.ones(p.shape[0], bool))
    src = tree["src"]
    inj = np.where((src >= 0)[:, None], p[np.maximum(src, 0)], 0.0)
    xw = None if edge_x is None else 2.0 * hr.to_pos(tree, np.asarray(edge_x, np.float64))
    return tree, inj, xw


@pytest.mark.parametrize("r,load,vset2", [(0.05, 1.0, 1.0), (0.3, 0.5, 1.0), (1e-3, 40.0, 1.0609), (0.02, -3.0, 1.0)])
def test_single_line_closed_form(r, load, vset2):
    """One line, one load, active only: u is the larger root of u^2 - (vset2 - w P) u + w^2 P^2 / 4 = 0."""
    tree, inj, _ = positions(np.array([-1]), np.array([r]), np.array([0]), np.array([[load]]))
    s = pf.solve(tree, 1, inj, vset2, tol=1e-16, max_iter=200, stall=True)
    w = 2.0 * r
    b = vset2 - w * load
    want = 0.5 * (b + np.sqrt(b * b - w * w * load * load))
    assert s["status"][0] == 0
    assert abs(s["u"][0, 0] - want) <= 1e-13 * want, (s["u"][0, 0], want)
    assert abs(s["lp"][0, 0] - r * load * load / want) <= 1e-13 * abs(r * load * load / want)
    assert s["P"][0, 0] == load


def random_tree(n, seed, with_x):
    rng = np.random.default_rng(100 * n + seed)
    parent = np.full(n, -1, np.int64)
    for i in range(1, n):
        parent[i] = rng.integers(-1, i) if rng.random() < 0.9 else -1
    er = rng.uniform(0.5, 1.5, n)
    er[rng.random(n) < 0.1] = 0.0
    ex = 0.5 * er * rng.uniform(0.5, 1.5, n) if with_x else None
    rows = np.flatnonzero(rng.random(n) < 0.8)
    cons = np.full(n, -1, np.int64)
    cons[rows] = np.arange(len(rows))
    p = rng.uniform(-0.3, 1.0, (max(len(rows), 1), 1))
    return parent, er, ex, cons, p


def whole_equations(parent, er, ex, node_p, node_q, vset2):
    """The branch-flow equations in the caller's node order, nothing of scans: z = (P, Q, u) -> the residuals of the flow
    balances and of u_child = u_parent - 2 (r P_send + x Q_send) + (r^2 + x^2) cur, P_send = P + r cur."""
    n = len(parent)
    kids = [np.flatnonzero(parent == i) for i in range(n)]

    def f(z):
        P, Q, u = z[:n], z[n:2 * n], z[2 * n:]
        cur = (P * P + Q * Q) / u
        Ps, Qs = P + er * cur, Q + ex * cur
        out = np.empty(3 * n)
        for i in range(n):
            out[i] = P[i] - (node_p[i] + Ps[kids[i]].sum())
            out[n + i] = Q[i] - (node_q[i] + Qs[kids[i]].sum())
            up = vset2 if parent[i] < 0 else u[parent[i]]
            out[2 * n + i] = u[i] - (up - 2.0 * (er[i] * Ps[i] + ex[i] * Qs[i]) + (er[i] ** 2 + ex[i] ** 2) * cur[i])
        return out
    return f


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("n", [8, 19, 60])
def test_solve_agrees_with_a_root_finder_on_random_trees(n, with_x):
    from scipy.optimize import root
    for seed in range(3):
        parent, er, ex, cons, p = random_tree(n, seed, with_x)
        tan_phi = np.tan(np.arccos(0.95)) if with_x else 0.0
        tree, inj, xw = positions(parent, er, cons, p, ex)
        lin = pf.solve(tree, n, inj, 1.0, xw, tan_phi, max_iter=1)
        drop = 1.0 - lin["u_lin"]
        s = 0.15 / np.abs(drop).max()                              # (the deepest linear drop is 0.15)
        sol = pf.solve(tree, n, inj * s, 1.0, xw, tan_phi, tol=1e-15, max_iter=100, stall=True)
        assert sol["status"][0] == 0 and sol["rho"][0] <= 0.5
        node_p = np.zeros(n)
        node_p[cons >= 0] = p[cons[cons >= 0], 0] * s
        x0 = np.concatenate([hr.to_nodes(tree, sol["P_lin"], n)[:, 0], tan_phi * hr.to_nodes(tree, sol["P_lin"], n)[:, 0],
                             hr.to_nodes(tree, sol["u_lin"], n)[:, 0]])
        f = whole_equations(parent, er, np.zeros(n) if ex is None else ex, node_p, tan_phi * node_p, 1.0)
        r = root(f, x0, method="hybr", tol=1e-15)
        assert np.abs(f(r.x)).max() <= 1e-12, r.message
        u = hr.to_nodes(tree, sol["u"], n)[:, 0]
        err = np.abs(u - r.x[2 * n:]).max()
        print(f"n={n} x={with_x} seed={seed}: |u - root| {err:.3e}, passes {sol['iters'][0]}, rho {sol['rho'][0]:.3f}")
        assert err <= 1e-10 * 1.0
        assert np.abs(hr.to_nodes(tree, sol["P"], n)[:, 0] - r.x[:n]).max() <= 1e-10


@pytest.fixture(scope="module")
def golden_case(golden):
    """The 121144 feeder with the x fixture laid on the graph's edges, read back by lpsolver.feeder_reactances as
    REVS.study(powerflow=True) reads it: per tree node, the reactance of the edge above it."""
    from test_network_host import golden_tree
    from revs_admm_amd.lpsolver import feeder_reactances
    z, _ = golden
    g, res, _, (par, er, cons), child, _ = golden_tree(golden)
    assert feeder_reactances(g, res) is None                       # (no edge carries an x yet)
    x = np.load(XFIX)["edge_x"]
    for (u, v), xv in zip(list(g.edges), x):
        g.edges[u, v]["x"] = float(xv)
    ex = feeder_reactances(g, res)
    assert ex.shape == er.shape and np.array_equal(ex[child], x)
    return par, er, cons, np.asarray(z["dis_a90_r4800_P_res"], np.float64), ex


def test_x_fixture_is_numbers_only():
    z = np.load(XFIX)
    assert os.path.getsize(XFIX) < 16384 and z.files == ["edge_x"]
    assert z["edge_x"].shape == (1691,) and z["edge_x"].dtype == np.float64 and np.isfinite(z["edge_x"]).all()
    assert (z["edge_x"] >= 0).all()


# What solve() gives on the 121144 feeder under the stored distributed schedule, vset = 1, over the residence rows of all 24
# slots: (cells at or below 0.95 by branch flow, by the linear model; at or below 0.92 likewise; the largest per-node
# volt_lin - volt; the lowest voltage by branch flow and by the linear model).
GOLDEN_ACTIVE = dict(le95=(195, 171), le92=(20, 18), err_max=0.0065, vmin=(0.8764, 0.8829))


def golden_figures(par, er, cons, p, ex, power_factor):
    tree, inj, xw = positions(par, er, cons, p, ex)
    tan_phi = np.tan(np.arccos(power_factor)) if ex is not None else 0.0
    sol = pf.solve(tree, len(par), inj, 1.0, xw, tan_phi, tol=1e-12, max_iter=32)
    rows = hr.to_pos(tree, cons >= 0, False)
    v, vl = np.sqrt(sol["u"]), np.sqrt(sol["u_lin"])
    fig = dict(le95=(int((v[rows] <= 0.95).sum()), int((vl[rows] <= 0.95).sum())),
               le92=(int((v[rows] <= 0.92).sum()), int((vl[rows] <= 0.92).sum())),
               err_max=float((vl - v)[hr.to_pos(tree, np.ones(len(par), bool), False)].max()),
               vmin=(float(v[rows].min()), float(vl[rows].min())))
    return sol, fig


def test_golden_feeder_active_only(golden_case):
    par, er, cons, p, _ = golden_case
    sol, fig = golden_figures(par, er, cons, p, None, 1.0)
    print("121144, dis_a90_r4800, active only:", fig, "passes", sol["iters"].max(), "rho", sol["rho"].max())
    assert (sol["status"] == 0).all() and sol["iters"].max() <= 10 and sol["rho"].max() <= 0.5
    assert fig["le95"] == GOLDEN_ACTIVE["le95"] and fig["le92"] == GOLDEN_ACTIVE["le92"]
    assert abs(fig["err_max"] - GOLDEN_ACTIVE["err_max"]) < 5e-5
    assert abs(fig["vmin"][0] - GOLDEN_ACTIVE["vmin"][0]) < 5e-5 and abs(fig["vmin"][1] - GOLDEN_ACTIVE["vmin"][1]) < 5e-5


# the same with the x fixture and power_factor = 0.95 (the linear side then carries the reactive term xw Q)
GOLDEN_PF95 = dict(le95=(255, 229), le92=(33, 27), err_max=0.0074, vmin=(0.8706, 0.8756))


def test_golden_feeder_with_reactances(golden_case):
    par, er, cons, p, ex = golden_case
    sol, fig = golden_figures(par, er, cons, p, ex, 0.95)
    print("121144, dis_a90_r4800, x fixture, pf 0.95:", fig, "passes", sol["iters"].max(), "rho", sol["rho"].max())
    assert (sol["status"] == 0).all() and sol["iters"].max() <= 10 and sol["rho"].max() <= 0.5
    assert fig["le95"] == GOLDEN_PF95["le95"] and fig["le92"] == GOLDEN_PF95["le92"]
    assert abs(fig["err_max"] - GOLDEN_PF95["err_max"]) < 5e-5
    assert abs(fig["vmin"][0] - GOLDEN_PF95["vmin"][0]) < 5e-5 and abs(fig["vmin"][1] - GOLDEN_PF95["vmin"][1]) < 5e-5
