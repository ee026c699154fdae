"""The power-flow report on the GPU (revs_net_powerflow; powerflow.report_for_tree, AdmmEngine.powerflow_report,
AdmmEnsemble.powerflow_reports, REVS.study(powerflow=)) against tests/powerflow_ref.py.

Preconditions, asserted on solve() alone: every slot converges with a contraction factor rho <= 0.5.  Then a run that
stops at max |du| <= tol vset2 is within tol vset2 rho / (1 - rho) <= tol vset2 of the fixed point, and the state one pass
before it within tol vset2 / (1 - rho) <= 2 tol vset2; the scans add BOUND = 1e-12 times the largest drop.  So

    |u - u*| <= 2 tol vset2 + BOUND max |drop|                                                    (E_u)

with u* from solve() run until it stalls.  P and lp are held to the same bound propagated through their formulas: what is
left of the iteration in P and lp where the kernel may stop (solve()'s own passes iters - 1 .. iters + 1 against its
fixed point, measured on the reference alone) plus what E_u and BOUND max |P| move through lp = 0.5 w (P^2 + Q^2) / u and
through the subtree sums of lp (bounds() below).  The residuals of the three equations at every node, from the kernel's own
arrays and the parent array alone, are held to the same bounds.  The measured maxima are printed beside the bounds.

Records: every field of slot, node_day and day is bit for bit contract() fed the kernel's arrays (qloss_total, which no
output array rebuilds, against solve() within the bound of lp scaled by xw / w = 0.5); the summaries by check_summary's
rules."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import headroom_ref as hr
import powerflow_ref as pf
from test_gpu_losses import bits, forest_case, same, small_case
from test_gpu_network import BOUND, golden_net, ulps  # noqa: F401  (golden_net: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("volt", "volt_lin", "flow", "loss")
RECORDS = ("summary", "slot", "node_day", "day")
U = 2.0 ** -53
PF = 0.95
TAN = float(np.tan(np.arccos(PF)))


def positions(par, er, cons, p, edge_x):
    from revs_admm_amd.feeder import feeder_tree
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    src = tree["src"]
    inj = np.where((src >= 0)[:, None], p[np.maximum(src, 0)], 0.0)
    xw = None if edge_x is None else 2.0 * hr.to_pos(tree, np.asarray(edge_x, np.float64))
    return tree, inj, xw


def bounds(tree, star, run, xw, vset2, tol):
    """-> (E_u scalar, E_P, E_lp (n, T) by position) for the good slots of `star` (solve() to its stall, keep=True) and `run`
    (solve(tol)): see the module's docstring."""
    w = np.asarray(tree["w"], np.float64)[:, None]
    n, T = star["u"].shape
    drop = vset2 - star["u"]
    e_u = 2.0 * tol * vset2 + BOUND * np.nanmax(np.abs(drop))
    tr_P, tr_lp = np.zeros((n, T)), np.zeros((n, T))
    for t in range(T):
        hs = star["hist"][t]
        for k in range(max(int(run["iters"][t]) - 1, 1), min(int(run["iters"][t]) + 1, len(hs)) + 1):
            _, P, _, lp = hs[k - 1]
            tr_P[:, t] = np.maximum(tr_P[:, t], np.abs(P - star["P"][:, t]))
            tr_lp[:, t] = np.maximum(tr_lp[:, t], np.abs(lp - star["lp"][:, t]))
    P, Q, u, lp = star["P"], star["Q"], star["u"], star["lp"]
    e_P0 = BOUND * np.nanmax(np.abs(P)) + tr_P                      # the state the last pass's lp was formed from
    lo = u - e_u
    assert (lo[~np.isnan(lo)] > 0).all()
    sq = 2.0 * np.abs(P) * e_P0 + e_P0 * e_P0
    if xw is not None:
        e_Q0 = TAN * e_P0 + BOUND * np.nanmax(np.abs(Q))
        sq = sq + 2.0 * np.abs(Q) * e_Q0 + e_Q0 * e_Q0
    r_lp = 0.5 * w * sq / lo + np.abs(lp) * e_u / lo + 16 * U * np.abs(lp)
    e_lp = tr_lp + r_lp
    sub = np.stack([pf.flow_sums(tree, np.nan_to_num(r_lp[:, t])) for t in range(T)], axis=1)
    e_P = e_P0 + sub + r_lp
    return e_u, e_P, e_lp


def check_report(rep, par, er, cons, p, edge_x=None, power_factor=1.0, nodes=None, vmin=0.95, cost=None, slot_hours=None,
                 tol=1e-12, max_iter=32, vset=1.0, expect_bad=()):
    """One scenario's PowerFlowReport: the preconditions on solve(), the arrays against solve() to its stall within the
    bounds, the residuals of the equations, and every record against contract() on the report's own arrays."""
    n, T = len(par), p.shape[1]
    vset2 = vset * vset
    tree, inj, xw = positions(par, er, cons, p, edge_x)
    tan_phi = float(np.tan(np.arccos(power_factor))) if edge_x is not None else 0.0
    run = pf.solve(tree, n, inj, vset2, xw, tan_phi, tol=tol, max_iter=max_iter)
    star = pf.solve(tree, n, inj, vset2, xw, tan_phi, tol=1e-15, max_iter=100, stall=True, keep=True)
    good = run["status"] == 0
    assert np.flatnonzero(~good).tolist() == sorted(expect_bad), run["status"]
    assert (star["status"][good] == 0).all() and (run["rho"][good] <= 0.5).all() and (star["rho"][good] <= 0.5).all()
    # ---- statuses, iters, the NaN rule
    assert same(rep.slot["status"], run["status"]), (rep.slot["status"], run["status"])
    assert (np.abs(rep.slot["iters"][good] - run["iters"][good]) <= 1).all(), (rep.slot["iters"], run["iters"])
    names = ARRAYS + (("qflow",) if edge_x is not None else ())
    for k in names:
        a = getattr(rep, k)
        if k != "volt_lin":
            assert np.isnan(a[:, ~good]).all() and not np.isnan(a[:, good]).any(), k
    assert (rep.qflow is None) == (edge_x is None)
    # ---- pass 0: the linear model's side (solve()'s pass 0 within the scans' bound)
    vl = hr.to_pos(tree, rep.volt_lin)
    has = np.asarray(tree["order"]) < n
    fin = run["status"] != 1                                        # (every slot whose injections are finite, collapsed or not)
    if fin.any():
        b_lin = BOUND * np.abs(vset2 - star["u_lin"][:, fin]).max() + 4 * U * max(vset2, np.abs(star["u_lin"][:, fin]).max())
        at = has[:, None] & fin[None, :] & (star["u_lin"] > 1e-9)   # (well inside the root's domain; below it a NaN may stand)
        assert np.abs(vl * vl - star["u_lin"])[at].max() <= b_lin
        assert np.isnan(vl[has[:, None] & fin[None, :] & (star["u_lin"] < -b_lin)]).all()
    # ---- against the fixed point
    if good.any():
        e_u, e_P, e_lp = bounds(tree, star, run, xw, vset2, tol)
        v, P, lp = (hr.to_pos(tree, getattr(rep, k)) for k in ("volt", "flow", "loss"))
        d_u = np.abs(v * v - star["u"])[has][:, good]
        d_P, d_lp = np.abs(P - star["P"])[has][:, good], np.abs(lp - star["lp"])[has][:, good]
        b_u = e_u + 4 * U * vset2                                   # (the root and the square: two roundings of <= vset^2)
        print(f"n={n} T={T} x={edge_x is not None}: iters {rep.slot['iters'].tolist()} (solve {run['iters'].tolist()}), rho "
              f"{np.nanmax(run['rho'][good]):.3f}; |u-u*| {d_u.max():.3e} (bound {b_u:.3e}); |P-P*| {d_P.max():.3e} (largest "
              f"err/bound {(d_P / e_P[has][:, good]).max():.3e}); |lp-lp*| {d_lp.max():.3e} (largest err/bound "
              f"{(d_lp / np.maximum(e_lp[has][:, good], 1e-300)).max():.3e})")
        assert d_u.max() <= b_u
        assert (d_P <= e_P[has][:, good]).all() and (d_lp <= e_lp[has][:, good]).all()
        if edge_x is not None:
            # lq = lp xw / w line by line, so qloss_total moves by the lines' bounds on lp times xw / w, plus the sum's order
            wq = np.asarray(tree["w"], np.float64)
            assert not ((wq == 0) & (xw > 0)).any()
            ratio = np.where(wq > 0, xw / np.where(wq > 0, wq, 1.0), 0.0)[:, None]
            lq = np.where(has[:, None], star["lq"], 0.0)[:, good]
            d_q = np.abs(rep.slot["qloss_total"][good] - lq.sum(axis=0))
            b_q = (np.where(has[:, None], e_lp, 0.0) * ratio)[:, good].sum(axis=0) + 2 * tree["n"] * U * np.abs(lq).sum(axis=0)
            assert (d_q <= b_q).all(), (d_q, b_q)
        else:
            assert (rep.slot["qloss_total"][good] == 0.0).all()
        residuals(rep, par, er, edge_x, tan_phi, cons, p, vset2, good, tree, e_u, e_P, e_lp)
    # ---- the records, bit for bit contract() on the report's own arrays
    mask = None
    if nodes is not None:
        mk = np.zeros(n, bool)
        mk[np.asarray(nodes, np.int64)] = True
        mask = hr.to_pos(tree, mk, False)
    hours = 24.0 / T if slot_hours is None else slot_hours
    b = pf.contract(tree, n, hr.to_pos(tree, rep.volt), vl, hr.to_pos(tree, rep.loss), inj, rep.slot["iters"],
                    rep.slot["status"], vmin, mask, cost, hours)
    for k in ("loss_total", "delivered", "supplied", "volt_min", "err_max"):
        bits(rep.slot[k], b["slot"][k], k)
    for k in ("volt_min_index", "err_index", "n_below", "n_below_lin", "n_missed"):
        assert same(rep.slot[k], b["slot"][k]), (k, rep.slot[k], b["slot"][k])
    assert np.isnan(rep.slot["qloss_total"][~good]).all() and (rep.slot["reserved"] == 0).all()
    for t, r in enumerate(b["summary"]):
        g = rep.summary[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"]), (t, g, r)
        if r["count"] == 0:
            assert np.isnan(g["min"]) and np.isnan(g["median"]) and np.isnan(g["worst_value"]) and g["n_fliers"] == 0
            continue
        box = r["box"]
        for k in ("min", "max", "whisker_lo", "whisker_hi"):
            assert g[k] == box[k], (t, k, g[k], box[k])
        assert g["worst_value"] == r["worst_value"]
        for k in ("q1", "median", "q3"):
            assert ulps(g[k], box[k]) <= 2, (t, k, g[k], box[k])
        assert g["n_fliers"] == box["n_fliers"], (t, g, box)
    bits(rep.node_day["volt_min"], b["node_day"]["volt_min"], "node_day volt_min")
    for k in ("slot", "slots_below", "slots_missed"):
        assert same(rep.node_day[k], b["node_day"][k]), k
    for k in ("energy_lost", "energy_delivered", "cost", "volt_min"):
        bits(rep.day[k], b["day"][k], "day " + k)
    for k in ("volt_min_slot", "volt_min_index", "n_below", "n_below_lin", "n_missed", "iters_max", "n_bad_slots"):
        assert rep.day[k] == b["day"][k], (k, rep.day[k], b["day"][k])
    assert rep.converged == bool(good.all())
    assert len(rep.missed()) == int(b["node_day"]["slots_missed"].sum())       # (both over every node)
    assert rep.error.tobytes() == (rep.volt_lin - rep.volt).tobytes()
    return b, run


def residuals(rep, par, er, edge_x, tan_phi, cons, p, vset2, good, tree, e_u, e_P, e_lp):
    """Every node's three equations from the report's own arrays, in the caller's node order: nothing of scans."""
    n = len(par)
    par = np.asarray(par, np.int64)
    r = np.asarray(er, np.float64)[:, None]
    x = np.zeros_like(r) if edge_x is None else np.asarray(edge_x, np.float64)[:, None]
    node_p = np.zeros((n, p.shape[1]))
    node_p[cons >= 0] = p[cons[cons >= 0]]
    g = np.flatnonzero(good)
    V, P, L, node_p = rep.volt[:, g], rep.flow[:, g], rep.loss[:, g], node_p[:, g]
    Q = np.zeros_like(P) if edge_x is None else rep.qflow[:, g]
    u = V * V
    cur = (P * P + Q * Q) / u
    bu, bP, bL = e_u + 4 * U * vset2, hr.to_nodes(tree, e_P, n)[:, g], hr.to_nodes(tree, e_lp, n)[:, g]
    assert not ((r == 0) & (x > 0)).any()
    bLq = bL * np.where(r > 0, x / np.where(r > 0, r, 1.0), 0.0)    # (lq = lp x / r line by line)
    # the loss on the line above every node: the report's lp is the last pass's, r cur the final state's, each within bL
    res_l = np.abs(L - r * cur)
    assert (res_l <= 2.0 * bL).all(), (res_l / np.maximum(2.0 * bL, 1e-300)).max()
    # the flow balance with the children
    kids_p, kids_q, kids_b, kids_bq = (np.zeros_like(P) for _ in range(4))
    has_par = par >= 0
    np.add.at(kids_p, par[has_par], (P + L)[has_par])
    np.add.at(kids_q, par[has_par], (Q + x * cur)[has_par])
    np.add.at(kids_b, par[has_par], (bP + bL)[has_par])
    np.add.at(kids_bq, par[has_par], (2.0 * bLq)[has_par])
    res_p = np.abs(P - (node_p + kids_p))
    assert (res_p <= bP + kids_b).all(), (res_p / (bP + kids_b)).max()
    if edge_x is not None:
        res_q = np.abs(Q - (tan_phi * node_p + kids_q))
        b_q = kids_bq + BOUND * np.abs(Q).max() + 16 * U * (np.abs(Q) + np.abs(kids_q))
        assert (res_q <= b_q).all(), (res_q / b_q).max()
    # the voltage against the parent's
    up = np.where(has_par[:, None], u[np.maximum(par, 0)], vset2)
    want = up - 2.0 * (r * (P + r * cur) + x * (Q + x * cur)) + (r * r + x * x) * cur
    res_u = np.abs(u - want)
    b_v = 2.0 * bu + 4.0 * r * bL + 4.0 * x * bLq
    print(f"    residuals: loss {res_l.max():.3e}, balance {res_p.max():.3e}, voltage {res_u.max():.3e} (largest err/bound "
          f"{(res_u / b_v).max():.3e})")
    assert (res_u <= b_v).all()


def run(par, er, cons, p, expect_bad=(), **kw):
    from revs_admm_amd.powerflow import report_for_tree
    rep = report_for_tree(par, er, cons, p, **kw)
    check_report(rep, par, er, cons, p, expect_bad=expect_bad, **kw)
    return rep


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("M", [8, 2048, 4096, 8192, 8200, 16384])
def test_every_tree_shape_matches_the_restatements(gpu_lib, M, T, with_x):
    """One thread (8), 256 x 8, 512 x 8, 1024 x 8, the first 1024 x 16 size (8200 pads to 8208) and the largest, with a node
    mask and a tariff; xw = 0.5 w and a power factor of 0.95 where used.  Without xw, pass 0 carries the loss report's
    bits."""
    from revs_admm_amd.losses import report_for_tree as loss_report
    par, er, cons, p, _, _ = forest_case(M)
    p = p[:, :T].copy()
    rng = np.random.default_rng(M + T)
    nodes = np.flatnonzero(rng.random(M) < 0.6)
    rep = run(par, er, cons, p, edge_x=0.5 * er if with_x else None, power_factor=PF, nodes=nodes,
              cost=rng.uniform(0.05, 0.3, T), slot_hours=0.25, vmin=0.95)
    assert rep.converged and rep.summary["count"][0] == len(nodes) and rep.slot["err_max"][0] > 0
    assert (rep.slot["loss_total"] > 0).all() and (rep.volt <= rep.volt_lin + 1e-12).all()
    # S = 3 in the same shape: scenario 0 is the call above, the others single calls on their own rows, byte for byte
    from revs_admm_amd.powerflow import report_for_tree
    kw = dict(edge_x=0.5 * er if with_x else None, power_factor=PF, nodes=nodes, slot_hours=0.25)
    ps = np.stack([p, 0.5 * p, p[::-1].copy()])
    for s, got in enumerate(report_for_tree(par, er, cons, ps, **kw)):
        one = report_for_tree(par, er, cons, ps[s], **kw)
        for k in ARRAYS + ("summary", "slot", "node_day"):
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        if s == 0:
            assert got.volt.tobytes() == rep.volt.tobytes() and got.slot.tobytes() == rep.slot.tobytes()
    if not with_x:
        lin = loss_report(par, er, cons, p)
        assert (1.0 - lin.drop >= 0).all() and np.sqrt(1.0 - lin.drop).tobytes() == rep.volt_lin.tobytes()
        assert rep.slot["delivered"].tobytes() == lin.slot["delivered"].tobytes()
        # pass 0's flows and u: a call that stops behind pass 1 (a tol it cannot miss) reports the lp formed from them
        first = report_for_tree(par, er, cons, p, tol=1e6, max_iter=1)
        assert first.converged and first.slot["iters"].tolist() == [1] * T
        assert first.loss.tobytes() == (er[:, None] * ((lin.flow * lin.flow) / (1.0 - lin.drop))).tobytes()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("with_x", [False, True])
def test_scenario_grid_equals_single_calls(gpu_lib, S, with_x):
    """S x T = 5 on 300 nodes: every scenario against the restatements, its slice equal in bytes to the S = 1 call."""
    from revs_admm_amd.powerflow import report_for_tree
    par, er, cons, p, _, _, rng = small_case()
    f = rng.uniform(0.5, 1.0, p.shape[1])
    ps = np.stack([p, p * f, p[::-1].copy()])[:S]
    kw = dict(nodes=np.flatnonzero(rng.random(300) < 0.5), cost=rng.uniform(0.1, 0.3, 5), vmin=0.93,
              edge_x=0.5 * er if with_x else None, power_factor=PF)
    reps = report_for_tree(par, er, cons, ps, **kw)
    assert len(reps) == S
    for s, rep in enumerate(reps):
        check_report(rep, par, er, cons, ps[s], **kw)
        one = report_for_tree(par, er, cons, ps[s], **kw)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (s, k)
    only = report_for_tree(par, er, cons, ps[0], arrays=False, **kw)
    assert only.volt is None
    for k in RECORDS:
        assert getattr(only, k).tobytes() == getattr(reps[0], k).tobytes(), k


@functools.lru_cache(maxsize=None)
def late_collapse_scale(M):
    """The scale of the case's slot 0 (deepest linear drop 0.15) a little past the one at which solve() stops converging:
    there pass 0 still has every voltage and a later pass loses one.  Found on solve() alone, by bisection."""
    if M == 300:
        par, er, cons, p, _, _, _ = small_case()
    else:
        par, er, cons, p, _, _ = forest_case(M)
    tree, inj, _ = positions(par, er, cons, p[:, :1], None)
    lo, hi = 1.0, 8.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if pf.solve(tree, M, inj * mid, 1.0, max_iter=64)["status"][0] == 0 else (lo, mid)
    return hi * 1.05


@pytest.mark.parametrize("M", [300, 8200])
def test_statuses(gpu_lib, M):
    """Status 1: a NaN injection.  Status 2: a slot scaled until solve() collapses.  Status 3: max_iter = 2.  Each ends as
    an arithmetic outcome; the other slots of the call hold the bytes of the call without the bad ones."""
    from revs_admm_amd.powerflow import report_for_tree
    if M == 300:
        par, er, cons, p, _, _, _ = small_case()
        p = p[:, :4].copy()
    else:
        par, er, cons, p, _, _ = forest_case(M)
        p = np.concatenate([p, p[:, :1]], axis=1)
    clean = report_for_tree(par, er, cons, p)
    bad = p.copy()
    bad[M // 3, 1] = np.nan
    bad[:, 2] *= 8.0                                                # (a deepest linear drop of 1.2 > vset^2)
    rep = run(par, er, cons, bad, expect_bad=(1, 2))
    assert rep.slot["status"].tolist() == [0, 1, 2, 0] and rep.day["n_bad_slots"] == 2 and not rep.converged
    for k in ARRAYS:
        assert getattr(rep, k)[:, [0, 3]].tobytes() == getattr(clean, k)[:, [0, 3]].tobytes(), k
    assert rep.slot[[0, 3]].tobytes() == clean.slot[[0, 3]].tobytes()
    assert rep.summary[[0, 3]].tobytes() == clean.summary[[0, 3]].tobytes()
    assert np.isnan(rep.volt_lin[:, 2]).any() and np.isnan(rep.day["energy_lost"])
    # a slot that collapses only behind pass 0: the linear model still has every voltage
    tree, inj, _ = positions(par, er, cons, p, None)
    scale = late_collapse_scale(M)
    s = pf.solve(tree, M, inj[:, :1] * scale, 1.0, max_iter=64)
    assert s["status"][0] == 2 and s["iters"][0] >= 1 and (s["u_lin"][np.asarray(tree["order"]) < M, 0] > 0).all()
    late = p.copy()
    late[:, 2] = p[:, 0] * scale
    rep2 = run(par, er, cons, late, max_iter=64, expect_bad=(2,))
    assert rep2.slot["status"].tolist() == [0, 0, 2, 0] and not np.isnan(rep2.volt_lin[:, 2]).any()
    assert rep2.slot["iters"][2] >= 1
    # max_iter = 2: no slot converges to 1e-12 in two passes
    rep3 = run(par, er, cons, p, max_iter=2, expect_bad=(0, 1, 2, 3))
    assert rep3.slot["status"].tolist() == [3] * 4 and rep3.slot["iters"].tolist() == [2] * 4
    assert rep3.volt_lin.tobytes() == clean.volt_lin.tobytes() and np.isnan(rep3.volt).all()


GOLDEN = {False: dict(le95=(195, 171), le92=(20, 18), err_max=0.0065), True: dict(le95=(255, 229), le92=(33, 27), err_max=0.0074)}


@pytest.mark.parametrize("with_x", [False, True])
def test_golden_feeder(gpu_lib, golden, golden_net, with_x):
    """The 121144 feeder, T = 24, under the stored distributed schedule: the counts and the largest error of the host
    test (tests/test_powerflow_host.py) come back from the device, over the residence rows."""
    from test_network_host import golden_tree
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    p = np.asarray(z["dis_a90_r4800_P_res"], np.float64)
    ex = None
    if with_x:
        ex = np.zeros(len(par))
        ex[golden_tree(golden)[4]] = np.load(os.path.join(HERE, "golden", "revs_121144_x.npz"))["edge_x"]
    rows = np.flatnonzero(cons >= 0)
    want = GOLDEN[with_x]
    for k, vmin in (("le95", 0.95), ("le92", 0.92)):
        # (the reference counts "at or below": vmin is the next double above the band)
        rep = run(par, er, cons, p, edge_x=ex, power_factor=PF, nodes=rows, vmin=float(np.nextafter(vmin, 1.0)),
                  cost=np.asarray(z["tariff_shift6"], np.float64), slot_hours=1.0)
        assert (int(rep.day["n_below"]), int(rep.day["n_below_lin"])) == want[k], (k, rep.day)
        assert rep.day["n_missed"] == want[k][0] - want[k][1]       # (the branch-flow voltage is never above the linear one)
    full = run(par, er, cons, p, edge_x=ex, power_factor=PF)
    assert abs(full.slot["err_max"].max() - want["err_max"]) < 5e-5 and full.converged and full.day["iters_max"] <= 10
    print(f"121144 x={with_x}: below 0.95 {want['le95']}, err_max {full.slot['err_max'].max():.5f}, lowest volt "
          f"{rep.day['volt_min']:.4f}, lost {full.day['energy_lost']:.1f} of {full.day['energy_delivered']:.1f} delivered")


def _small_workload():
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(2000, 24, n_nodes=64, seed=3, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    return w


def test_engine_powerflow_report(gpu_lib):
    """After a short streaming run: powerflow_report() of the schedule equals report_for_tree on the same node sums; the
    run's state keeps its bytes."""
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.powerflow import report_for_tree
    w = _small_workload()
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run(3)
    e.run_steps(10)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    ex = 0.5 * np.asarray(w.edge_r, np.float64)
    rep = e.powerflow_report(edge_x=ex, power_factor=PF)
    g = np.zeros((w.M, 24))
    np.add.at(g, w.node_of, w.load.astype(np.float64) + e.result()[0].astype(np.float64))
    cost = w.cost.astype(np.float64)
    sums = e.network_report(arrays=False).node_sums                # (the engine's own node sums of the schedule)
    one = report_for_tree(w.parent, w.edge_r, np.arange(w.M), sums, edge_x=ex, power_factor=PF, vset=w.vset, cost=cost)
    for k in ARRAYS + ("qflow",) + RECORDS:
        assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), k
    assert np.abs(sums - g).max() <= 1e-12 * np.abs(g).max()
    g = sums
    check_report(rep, np.asarray(w.parent), np.asarray(w.edge_r, np.float64), np.arange(w.M), g, edge_x=ex, power_factor=PF,
                 vset=w.vset, cost=cost)
    base = e.powerflow_report(profile=w.load, arrays=False)
    assert base.volt is None and base.day["energy_lost"] > 0 and base.qflow is None
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    e.run_steps(2)


def test_ensemble_powerflow_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.powerflow_reports()[s] holds the bytes of a single engine's report on scenario s."""
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    ex = 0.5 * np.asarray(w.edge_r, np.float64)
    reps = ens.powerflow_reports(edge_x=ex, power_factor=PF, vmin=0.97)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.powerflow_report(edge_x=ex, power_factor=PF, vmin=0.97)
        for k in ARRAYS + ("qflow",) + RECORDS:
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert one.converged and np.isfinite(one.day["cost"])


SHARD_CASE = dict(name="pf", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports hold
    the one-rank bytes."""
    sys.path.insert(0, HERE)
    from network_worker import engine
    from powerflow_worker import reports
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_volt"]).all()
    port = 29900 + (os.getpid() + 1231) % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "powerflow_worker.py"), str(path)], stdout=log,
                                       stderr=subprocess.STDOUT, env=env), log))
    rcs = []
    for p, log in procs:
        try:
            rcs.append(p.wait(timeout=600))
        except subprocess.TimeoutExpired:
            p.kill()
            rcs.append(-9)
        log.close()
    logs = "\n".join((tmp_path / f"w{r}.log").read_text()[-3000:] for r in range(2))
    assert rcs == [0, 0], logs
    for r in range(2):
        got = np.load(tmp_path / f"pf_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


def test_study_fills_powerflow(gpu_lib, golden):
    """REVS.study(powerflow=True) on the 121144 feeder with the x fixture on the graph's edges: StudyReport.powerflow[s]
    holds the bytes of report_for_tree on the report's own row s with the reactances feeder_reactances reads; the default
    leaves it None."""
    from test_gpu_losses import _study_inputs
    from revs_admm_amd.lpsolver import feeder_reactances
    from revs_admm_amd.powerflow import report_for_tree
    from revs_admm_amd.revs_fixture import REVS
    tariff, all_homes, dist, com, (parent, edge_r, cons_of) = _study_inputs(golden)
    x = np.load(os.path.join(HERE, "golden", "revs_121144_x.npz"))["edge_x"]
    for (u, v), xv in zip(list(dist.edges), x):
        dist.edges[u, v]["x"] = float(xv)
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    edge_x = feeder_reactances(dist, res)
    assert edge_x is not None and edge_x.shape == edge_r.shape and np.sort(edge_x).tobytes() == np.sort(x).tobytes()
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234,), methods=("individual", "uncontrolled"), arrays=True)
    assert REVS().study(tariff, all_homes, dist, com, **dict(grid, methods=("uncontrolled",)))[1].powerflow is None
    labels, rep = REVS().study(tariff, all_homes, dist, com, powerflow=dict(power_factor=PF), **grid)
    assert len(rep.powerflow) == len(labels) == 2
    pos = {n: i for i, n in enumerate(nonsub)}
    for s, got in enumerate(rep.powerflow):
        one = report_for_tree(parent, edge_r, cons_of, rep.node_p[s], edge_x=edge_x, power_factor=PF,
                              nodes=[pos[h] for h in com], cost=np.asarray(tariff, np.float64))
        for k in ARRAYS + ("qflow",) + RECORDS:
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert got.converged and got.day["n_below"] >= got.day["n_below_lin"]
