"""The headroom report on the GPU (revs_net_headroom; headroom.report_for_tree, AdmmEngine.headroom_report,
AdmmEnsemble.headroom_reports) against tests/headroom_ref.py: bit for bit the contract (b) fed the kernel's own drop /
flow arrays, which are held to the dense form with test_gpu_network.py's bounds and equal revs_net_report's flow in
bytes; the summaries by check_summary's rules (== for order statistics and counts, <= 2 ulp for the interpolated
quartiles); the day records; every tree shape and the code paths behind them.

The issue's evening clause (the distributed schedule leaves no more nodes short of 4.8 kW in slots 14-16 than the
individual one) is NOT asserted: the numpy restatement on the stored results says otherwise -- 469 / 461 / 182 nodes
short under the distributed schedule against 180 / 174 / 165 under the individual one at vset = 1.0 (158 / 158 / 6
against 157 / 157 / 6 at 1.03); the distributed schedule moves charging INTO those hours."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import headroom_ref as hr
from test_gpu_network import BOUND, dense_of_forest, golden_net, synthetic_forest, ulps  # noqa: F401  (golden_net: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def check_report(rep, par, er, cons, p, rating, limit_nodes, nodes, vset, vmin, need, dense=True):
    """One scenario's HeadroomReport against (b) on its own drop / flow; drop / flow against the dense form."""
    from revs_admm_amd.feeder import feeder_tree, headroom_aux
    n = len(par)
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    aux = headroom_aux(tree)
    if dense:
        P = np.zeros((n, p.shape[1]))
        P[np.flatnonzero(np.asarray(cons) >= 0)] = p[np.asarray(cons)[np.asarray(cons) >= 0]]
        fin = np.isfinite(P).all(axis=0)
        F, RP = dense_of_forest(np.asarray(par), np.asarray(er, np.float64), P[:, fin])
        eF, eV = BOUND * np.abs(F).max(), BOUND * np.abs(RP).max()
        print(f"flow err {np.abs(rep.flow[:, fin] - F).max():.3e} (bound {eF:.3e}), drop err "
              f"{np.abs(rep.drop[:, fin] - RP).max():.3e} (bound {eV:.3e})")
        assert np.abs(rep.flow[:, fin] - F).max() <= eF and np.abs(rep.drop[:, fin] - RP).max() <= eV
    rt = np.zeros(n) if rating is None else np.nan_to_num(np.asarray(rating, np.float64), nan=0.0)
    rows = np.asarray(cons) >= 0

    def mask(sel):                                       # None: the nodes that carry a row, the report's default
        if sel is None:
            return rows.copy()
        mk = np.zeros(n, bool)
        mk[np.asarray(sel, np.int64)] = True
        return mk

    lim, keep = mask(limit_nodes), mask(nodes)
    src_rows = np.where(tree["src"] >= 0, tree["src"], 0)
    nan_slot = ~np.isfinite(np.where((tree["src"] >= 0)[:, None], p[src_rows], 0.0)).all(axis=0)
    dmax = vset * vset - vmin * vmin
    with np.errstate(invalid="ignore"):
        head, at, kind = hr.contract(aux, hr.to_pos(tree, lim, False), hr.to_pos(tree, rep.drop), hr.to_pos(tree, rep.flow),
                                     hr.to_pos(tree, rt), dmax, nan_slot)
    want = hr.to_nodes(tree, head, n)
    assert np.array_equal(rep.headroom, want, equal_nan=True), np.nanmax(np.abs(rep.headroom - want))
    assert rep.headroom[~np.isnan(want)].tobytes() == want[~np.isnan(want)].tobytes()
    words = hr.to_nodes(tree, hr.limiter_words(tree, at, kind, n), n)
    got = np.where(rep.limiter_node < 0, -1, rep.limiter_node | (rep.limiter_kind << 30))
    assert np.array_equal(got, words), np.argwhere(got != words)[:5]
    for t, r in enumerate(hr.summary(rep.headroom, keep, need)):
        g = rep.summary[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"], g["reserved"][0]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"], r["n_unlimited"]), (t, g, r)
        if r["count"] == 0:
            assert np.isnan(g["min"]) and np.isnan(g["median"]) and np.isnan(g["worst_value"]) and g["n_fliers"] == 0
            continue
        b = r["box"]
        for k in ("min", "max", "whisker_lo", "whisker_hi"):
            assert g[k] == b[k], (t, k, g[k], b[k])
        assert g["worst_value"] == r["worst_value"]
        for k in ("q1", "median", "q3"):
            assert ulps(g[k], b[k]) <= 2, (t, k, g[k], b[k])
        assert g["n_fliers"] == b["n_fliers"], (t, g, b)
    mn, slot, short = hr.day(rep.headroom, need)
    assert np.array_equal(rep.day["min"], mn, equal_nan=True)
    assert np.array_equal(rep.day["slot"], slot) and np.array_equal(rep.day["n_short"], short)
    return tree


def run(par, er, cons, p, rating=None, limit_nodes=None, nodes=None, vset=1.0, vmin=0.95, need=4.8, dense=True):
    from revs_admm_amd.headroom import report_for_tree
    rep = report_for_tree(par, er, cons, p, need=need, rating=rating, limit_nodes=limit_nodes, nodes=nodes, vset=vset,
                          vmin=vmin)
    check_report(rep, par, er, cons, p, rating, limit_nodes, nodes, vset, vmin, need, dense)
    return rep


def forest_case(M, T, seed, unrated=0.15):
    """A forest of M nodes, every node a row, loads scaled so that the deepest drop is 0.09 (drop_max is 0.0975: a few
    per cent of slack at the worst node), ratings around the largest flows, some lines unrated."""
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed)
    p = rng.uniform(0.0, 4.0, (M, T))
    F, RP = dense_of_forest(par, er, p)
    s = 0.09 / np.abs(RP).max()
    rating = rng.uniform(0.3, 2.0, M) * np.abs(F * s).max()
    rating[rng.random(M) < unrated] = np.nan
    return par, er, cons, p * s, rating, rng


@pytest.mark.parametrize("M,T", [(13, 1), (2056, 2), (4104, 2), (8200, 2)])
def test_every_tree_shape_matches_the_contract(gpu_lib, M, T):
    """256 x 8 (13 nodes padded to 16), 512 x 8, 1024 x 8 and 1024 x 16 (8200 nodes pad to 8208), with a limit mask, an
    output mask and unrated lines; the flow equals revs_net_report's in bytes, the drop its voltage within the root."""
    from revs_admm_amd.network import report_for_tree as net_report
    par, er, cons, p, rating, rng = forest_case(M, T, seed=M)
    limit_nodes = np.flatnonzero(rng.random(M) < 0.6)
    nodes = np.flatnonzero(rng.random(M) < 0.7)
    rep = run(par, er, cons, p, rating, limit_nodes, nodes)
    assert np.isfinite(rep.headroom).any() and (rep.limiter_kind == 0).any()
    assert M < 2000 or (rep.limiter_kind == 1).any()              # (both kinds of limiter on every large shape)
    net = net_report(par, er, cons, p, rating=rating)
    assert net.flow.tobytes() == rep.flow.tobytes()
    assert (ulps(np.sqrt(1.0 - rep.drop), net.volt) <= 1).all()


def chain(n, r=1.0):
    return np.arange(-1, n - 1), np.full(n, r), np.arange(n)


def test_hand_cases(gpu_lib):
    """The host test's hand cases at T = 3 (three load levels: slack, none, beyond the limit)."""
    lv = np.array([[0.5, 1.0, 2.0]])
    # a chain of 8, a star, two roots plus padding
    run(*chain(8, 0.5), np.arange(8)[:, None] / 64 * lv, vset=2.0, vmin=1.0, need=0.1)
    run(np.full(6, -1), np.ones(6), np.arange(6), np.arange(1.0, 7.0)[:, None] / 32 * lv, need=0.1)
    rep = run(np.array([-1, 0, 0, -1, 3]), np.ones(5), np.arange(5), np.full((5, 1), 0.01) * lv, need=0.01)
    assert np.isfinite(rep.headroom).all()
    # zero-resistance edges all the way and no rating: +inf, limiter -1, nothing to summarise
    rep = run(np.array([-1, 0, 1]), np.zeros(3), np.arange(3), np.ones((3, 1)) * lv)
    assert np.isinf(rep.headroom).all() and (rep.limiter_node == -1).all() and (rep.summary["count"] == 0).all()
    assert (rep.summary["reserved"][:, 0] == 3).all() and (rep.day["slot"] == 0).all() and np.isinf(rep.day["min"]).all()
    # an unrated lateral off a rated trunk, no limit node below it: the trunk's thermal room alone
    rep = run(np.array([-1, 0, 0]), np.array([1.0, 0.0, 0.0]), np.array([0, 1, 2]), np.ones((3, 1)) * lv,
              rating=[8.0, np.nan, np.nan], limit_nodes=[], nodes=[0, 1, 2], need=3.0)
    assert np.array_equal(rep.headroom, np.tile(8.0 - 3.0 * lv, (3, 1))) and (rep.limiter_kind == 1).all()
    # a limit node below vmin (drop 8 > 7), a slack exactly 0 (drop 8 = 8): 0, the limiter kept at the top of the chain
    for vset, vmin in ((4.0, 3.0), (3.0, 1.0)):                   # (drop_max = vset^2 - vmin^2 = 7, 8 exactly)
        rep = run(*chain(4), np.array([[0.0], [0.0], [0.0], [1.0]]), vset=vset, vmin=vmin)
        assert (rep.headroom == 0.0).all() and (rep.limiter_node == 0).all() and (rep.limiter_kind == 0).all()
    # the tie rules, from powers of two (chain of 3, w = 1, no load; drop_max = 4)
    par, er, cons = chain(3, 0.5)
    z = np.zeros((3, 3))
    tie = lambda **kw: run(par, er, cons, z, vset=2.5, vmin=1.5, **kw)     # (6.25 - 2.25 = 4 exactly)
    rep = tie(rating=[4.0, 0, 0], limit_nodes=[0])                 # voltage == thermal at node 0: voltage first
    assert (rep.headroom == 4.0).all() and (rep.limiter_node == 0).all() and (rep.limiter_kind == 0).all()
    rep = tie(rating=[2.0, 2.0, 0], limit_nodes=[], nodes=[0, 1, 2])   # two ancestors tie: the shallowest
    assert (rep.headroom == 2.0).all() and (rep.limiter_node == 0).all() and (rep.limiter_kind == 1).all()
    rep = tie(rating=[2.0, 0, 0], limit_nodes=[1])                 # node 1's voltage term == node 0's thermal: node 0
    assert (rep.headroom == 2.0).all() and (rep.limiter_node == 0).all() and (rep.limiter_kind == 1).all()


def test_chain_of_depth_2048(gpu_lib):
    """One lateral of 2048 nodes: 11 rounds of jumps where a level-wise pass would take 2047 steps.  The launch runs in
    a child process with its own time limit."""
    code = ("import numpy as np, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from revs_admm_amd.headroom import report_for_tree\n"
            "n = 2048; rng = np.random.default_rng(4)\n"
            "p = rng.uniform(0.0, 1.0, (n, 1)); p *= 0.09 / (2.0 * np.cumsum(np.cumsum(p[::-1, 0])[::-1] * 1e-3)).max()\n"
            "rep = report_for_tree(np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n), p, need=1e-6)\n"
            "np.savez(sys.argv[1], p=p, headroom=rep.headroom, node=rep.limiter_node, kind=rep.limiter_kind, drop=rep.drop,\n"
            "         flow=rep.flow, summary=rep.summary.view(np.uint8), day=rep.day.view(np.uint8))\n"
            % (HERE, os.path.dirname(HERE)))
    import tempfile
    from revs_admm_amd._lib import HEADROOM_DAY_DTYPE
    from revs_admm_amd.headroom import HeadroomReport
    from revs_admm_amd.network import SUMMARY_DTYPE
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "chain.npz")
        r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        g = np.load(out)
        rep = HeadroomReport(g["headroom"], g["node"], g["kind"], g["summary"].view(SUMMARY_DTYPE),
                             g["day"].view(HEADROOM_DAY_DTYPE), 1e-6, 1.0, 0.95, g["drop"], g["flow"])
        p = g["p"]
    n = 2048
    check_report(rep, np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n), p, None, None, None, 1.0, 0.95, 1e-6)
    assert (rep.limiter_kind == 0).all() and (np.diff(rep.headroom[:, 0]) <= 0).all()


def test_scenario_grid_equals_single_calls(gpu_lib):
    """S = 3 x T = 5 on 300 nodes with masks and unrated lines: every scenario against (b), and its slice equal in
    bytes to the S = 1 call on that scenario."""
    from revs_admm_amd.headroom import report_for_tree
    par, er, cons, p, rating, rng = forest_case(300, 5, seed=300, unrated=0.3)
    ps = np.stack([p, p * rng.uniform(0.5, 1.1, p.shape), p[::-1].copy()])
    limit_nodes, nodes = np.flatnonzero(rng.random(300) < 0.6), np.flatnonzero(rng.random(300) < 0.5)
    kw = dict(need=0.002, rating=rating, limit_nodes=limit_nodes, nodes=nodes)
    reps = report_for_tree(par, er, cons, ps, **kw)
    assert len(reps) == 3
    for s, rep in enumerate(reps):
        check_report(rep, par, er, cons, ps[s], rating, limit_nodes, nodes, 1.0, 0.95, 0.002)
        one = report_for_tree(par, er, cons, ps[s], **kw)
        for k in ("headroom", "limiter_node", "limiter_kind", "drop", "flow", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (s, k)
    assert reps[0].summary["n_violations"].max() > 0 and reps[0].tightest is not None
    assert np.array_equal(reps[0].fits, reps[0].summary["count"] - reps[0].n_short)


@pytest.mark.parametrize("tag", ["dis_a90_r4800", "ind_a90_r4800"])
def test_stored_results_of_the_reference(gpu_lib, golden, golden_net, tag):
    """The 121144 feeder, T = 24, under the stored distributed and individual schedules with the lines' ratings: equal
    to (b).  (The evening clause of the issue is not asserted: see the module's docstring.)"""
    z, gn = golden[0], golden_net
    par, er, cons = gn["feeder"]
    rep = run(par, er, cons, z[tag + "_P_res"], gn["rating"], dense=False)
    P = np.zeros((gn["n"], 24))
    P[gn["rows"]] = z[tag + "_P_res"]
    F, RP = gn["to_node"](gn["A_inv"] @ P), gn["R"] @ P
    assert np.abs(rep.flow - F).max() <= BOUND * np.abs(F).max() and np.abs(rep.drop - RP).max() <= BOUND * np.abs(RP).max()
    assert (rep.summary["count"] + rep.summary["reserved"][:, 0] == 1126).all() and (rep.summary["n_nan"] == 0).all()
    node, t, x = rep.tightest
    assert x == rep.headroom[node, t] == np.nanmin(rep.headroom[gn["rows"]])


def test_nan_slot(gpu_lib):
    """A non-finite injection in one slot of three: that slot reads NaN / -1 / count 0, the others are unaffected."""
    par, er, cons, p, rating, rng = forest_case(300, 3, seed=7)
    clean = run(par, er, cons, p, rating, need=0.002)
    for bad in (np.nan, np.inf):
        q = p.copy()
        q[17, 1] = bad
        rep = run(par, er, cons, q, rating, need=0.002, dense=False)
        assert np.isnan(rep.headroom[:, 1]).all() and (rep.limiter_node[:, 1] == -1).all() and (rep.limiter_kind[:, 1] == -1).all()
        assert rep.summary["count"][1] == 0 and rep.summary["n_nan"][1] == 300 and rep.summary["reserved"][1, 0] == 0
        for k in ("headroom", "limiter_node", "limiter_kind", "drop", "flow"):
            assert getattr(rep, k)[:, [0, 2]].tobytes() == getattr(clean, k)[:, [0, 2]].tobytes(), k
        assert rep.summary[[0, 2]].tobytes() == clean.summary[[0, 2]].tobytes()
        assert not np.isnan(rep.day["min"]).any() and (rep.day["slot"] != 1).all()
    q = np.full_like(p, np.nan)
    rep = run(par, er, cons, q, rating, need=0.002, dense=False)
    assert np.isnan(rep.day["min"]).all() and (rep.day["slot"] == -1).all() and (rep.day["n_short"] == 0).all()


def test_every_output_alone_and_summary_only(gpu_lib):
    """Each output with every other one NULL holds the bytes of the full call; arrays=False gives the same summary."""
    import ctypes as C
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.headroom import aux_on_device, position_mask, report_for_tree
    from revs_admm_amd.network import SUMMARY_DTYPE, side_arrays, tree_on_device
    par, er, cons, p, rating, rng = forest_case(300, 4, seed=12)
    full = report_for_tree(par, er, cons, p, need=0.002, rating=rating)
    only = report_for_tree(par, er, cons, p, need=0.002, rating=rating, arrays=False)
    assert only.headroom is None and only.limiter_node is None
    assert only.summary.tobytes() == full.summary.tobytes() and only.day.tobytes() == full.day.tobytes()
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    aux, _k2 = aux_on_device(dev, th)
    d_nop, d_rating, _ = side_arrays(dev, th, 300, rating, None)
    d_outm = position_mask(dev, th, 300, None)
    g = torch.from_numpy(p).to(dev)
    scratch = torch.empty(lib.revs_net_headroom_scratch(1, 4, th["n"]) // 8, dtype=torch.float64, device=dev)
    word = np.where(full.limiter_node < 0, -1, full.limiter_node | (full.limiter_kind << 30)).astype(np.int32)
    wants = [full.headroom, word, full.drop, full.flow, full.summary, full.day]
    sizes = [300 * 4 * 8, 300 * 4 * 4, 300 * 4 * 8, 300 * 4 * 8, 4 * SUMMARY_DTYPE.itemsize, 300 * _lib.HEADROOM_DAY_DTYPE.itemsize]
    for k in range(6):
        outs = [None] * 6
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = lib.revs_net_headroom(1, 300, 4, C.byref(tree), C.byref(aux), g.data_ptr(), d_rating.data_ptr(), None,
                                   d_outm.data_ptr(), d_nop.data_ptr(), 300, 1.0 - 0.95 ** 2, 0.002,
                                   *[None if o is None else o.data_ptr() for o in outs],
                                   scratch.data_ptr() if k >= 4 else None, None)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k


def _small_workload():
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(2000, 24, n_nodes=64, seed=3, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    return w


def test_engine_headroom_report(gpu_lib):
    """After a short streaming run: headroom_report() of the schedule and of a rule schedule against (b) and the dense
    form; `need` defaults to the largest charger rating; the run's state keeps its bytes."""
    from revs_admm_amd.engine import AdmmEngine
    w = _small_workload()
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run(3)
    e.run_steps(10)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    rating = np.random.default_rng(5).uniform(30.0, 400.0, w.M)
    rep = e.headroom_report(rating=rating)
    assert rep.need == float(w.homes["rating"][w.homes["ev"] != 0].max()) == float(np.float32(7.2))
    assert (rep.vset, rep.vmin) == (w.vset, w.vlow)
    has = np.bincount(w.node_of, minlength=w.M) > 0
    g = np.zeros((w.M, 24))
    np.add.at(g, w.node_of, w.load.astype(np.float64) + e.result()[0].astype(np.float64))
    check_report(rep, w.parent, w.edge_r, np.arange(w.M), g, rating, np.flatnonzero(has), np.flatnonzero(has), w.vset,
                 w.vlow, rep.need)
    prof = e.rule_schedule("uncontrolled")
    rule = e.headroom_report(profile=prof, need=4.8, rating=rating)
    prof_h = (prof if isinstance(prof, np.ndarray) else prof.cpu().numpy()[e.inv_perm]).astype(np.float64)
    g2 = np.zeros((w.M, 24))
    np.add.at(g2, w.node_of, prof_h)
    check_report(rule, w.parent, w.edge_r, np.arange(w.M), g2, rating, np.flatnonzero(has), np.flatnonzero(has), w.vset,
                 w.vlow, 4.8)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    e.run_steps(2)


def test_ensemble_headroom_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.headroom_reports()[s] holds the bytes of a single engine's report on scenario s; the headroom tensor
    can stay on the device."""
    import torch
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    rating = np.random.default_rng(6).uniform(30.0, 400.0, w.M)
    out = torch.zeros(3, w.M, 24, dtype=torch.float64, device=ens.dev)
    reps = ens.headroom_reports(need=4.8, rating=rating, add_load=False, out=out)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.headroom_report(profile=e.P_sch, need=4.8, rating=rating)
        for k in ("headroom", "limiter_node", "limiter_kind", "drop", "flow", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert out[s].cpu().numpy().tobytes() == one.headroom.tobytes()


SHARD_CASE = dict(name="head", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports --
    of the schedule after 4 iterations with the default `need`, and of a given profile -- hold the one-rank bytes."""
    sys.path.insert(0, HERE)
    from headroom_worker import reports
    from network_worker import engine
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_headroom"]).any()
    port = 29900 + os.getpid() % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "headroom_worker.py"), str(path)], stdout=log,
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
        got = np.load(tmp_path / f"head_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


def test_study_fills_headroom(gpu_lib, golden):
    """REVS.study(headroom=need) on the 121144 feeder, 2 seeds x {individual, uncontrolled}: StudyReport.headroom[s] holds
    the bytes of report_for_tree on the report's own row s, summarised over the community; the default leaves it None."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.headroom import report_for_tree
    from revs_admm_amd.lpsolver import feeder_of
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), methods=("individual", "uncontrolled"), arrays=True)
    labels, rep = REVS().study(tariff, all_homes, dist, com, headroom=4.8, **grid)
    assert REVS().study(tariff, all_homes, dist, com, **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].headroom is None
    assert len(rep.headroom) == len(labels) == 4
    parent, edge_r, cons_of = feeder_of(dist)[1]
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    pos = {n: i for i, n in enumerate(nonsub)}
    nodes = [pos[h] for h in com]
    for s, got in enumerate(rep.headroom):
        one = report_for_tree(parent, edge_r, cons_of, rep.node_p[s], need=4.8, nodes=nodes)
        for k in ("headroom", "limiter_node", "limiter_kind", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert (got.summary["count"] + got.summary["reserved"][:, 0] == len(com)).all() and got.need == 4.8
