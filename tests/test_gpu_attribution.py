"""The attribution report on the GPU (revs_net_attribution; attribution.report_for_tree, AdmmEngine.attribution_report,
AdmmEnsemble.attribution_reports, REVS.study(attribution=True)) against tests/attr_ref.py: bit for bit the contract fed
the kernel's own drop array -- sens, contrib, ev_contrib, the slot records with their six sums, the day records, the
summary's order statistics and counts; the interpolated quartiles within 2 ulp (check_summary's rule); drop equal to
revs_net_headroom's in bytes; every tree shape and the code paths behind them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attr_ref as ar
from test_gpu_network import synthetic_forest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLOT_FIELDS = ("drop_watch", "excess", "total", "ev_total", "class_total", "top_value", "top_index", "watch", "n_reach",
               "n_big", "n_can", "n_bad")


def same(a, b):
    """Equal in bytes, NaNs at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == b[~nan].tobytes()


def reference(rep, par, er, cons, p, ev, limit_nodes, nodes, classes, watch, vset, vmin, frac):
    """attr_ref.contract on the report's own drop, by position -> (tree, its result)."""
    from revs_admm_amd.feeder import feeder_tree, headroom_aux
    n = len(par)
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    aux = headroom_aux(tree)
    rows = lambda a: np.where((tree["src"] >= 0)[:, None], a[np.maximum(tree["src"], 0)], 0.0)

    def mask(sel):                                       # None: the nodes that carry a row, the report's default
        mk = np.zeros(n, bool)
        if sel is None:
            mk[:] = np.asarray(cons) >= 0
        else:
            mk[np.asarray(sel, np.int64)] = True
        return ar.to_pos(tree, mk, False)

    cls = None if classes is None else ar.to_pos(tree, np.asarray(classes, np.int64), 255)
    C = 0 if classes is None else int(np.asarray(classes).max()) + 1
    wpos = -1 if watch is None else int(np.flatnonzero(tree["order"] == watch)[0])
    with np.errstate(invalid="ignore"):
        out = ar.contract(tree, aux, n, rows(p), None if ev is None else rows(ev), ar.to_pos(tree, rep.drop),
                          vset * vset - vmin * vmin, frac, limit=None if limit_nodes is None else mask(limit_nodes),
                          out_mask=mask(nodes), cls=cls, C=C, watch_pos=wpos)
    return tree, out


def check_report(rep, par, er, cons, p, ev=None, limit_nodes=None, nodes=None, classes=None, watch=None, vset=1.0,
                 vmin=0.95, frac=0.01):
    n = len(par)
    tree, out = reference(rep, par, er, cons, p, ev, limit_nodes, nodes, classes, watch, vset, vmin, frac)
    for k in ("sens", "contrib") + (("ev_contrib",) if ev is not None else ()):
        want = ar.to_nodes(tree, out[k], n)
        assert same(getattr(rep, k), want), (k, np.nanmax(np.abs(getattr(rep, k) - want)))
    assert ev is not None or rep.ev_contrib is None
    for k in SLOT_FIELDS:
        assert same(rep.slot[k], out["slot"][k]), (k, rep.slot[k], out["slot"][k])
    assert not rep.slot["reserved"].any()
    ar.check_summary(rep.summary, out["summary"])
    for k in ("sum", "ev_sum", "peak", "peak_slot", "n_big"):
        assert same(rep.day[k], out["day"][k]), (k, np.flatnonzero(rep.day[k] != out["day"][k])[:5])
    ok = rep.slot["n_bad"] == 0
    assert same(rep.relief()[:, ok], ar.relief(rep.sens[:, ok], rep.slot["excess"][ok]))
    return out


def run(par, er, cons, p, ev=None, **kw):
    from revs_admm_amd.attribution import report_for_tree
    rep = report_for_tree(par, er, cons, p, ev, **kw)
    check_report(rep, par, er, cons, p, ev, **kw)
    return rep


def forest_case(M, T, seed, peaks=(0.11, 0.09), limit_nodes=None):
    """A forest of M nodes, every node a row, loads scaled slot by slot as test_gpu_headroom.forest_case scales them --
    the deepest drop among the limit nodes in slot t is peaks[t % 2] against drop_max = 0.0975, so the even slots have
    an excess -- and an EV part of random fractions of the injections."""
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed)
    p = rng.uniform(0.0, 4.0, (M, T))
    _, drop = tree_report_host(feeder_tree(par, er, cons, np.ones(M, bool)), p, M)
    top = (drop if limit_nodes is None else drop[limit_nodes]).max(axis=0)
    p = p * (np.array([peaks[t % 2] for t in range(T)]) / top)[None, :]
    return par, er, cons, p, p * rng.uniform(0.0, 1.0, p.shape), rng


@pytest.mark.parametrize("M,T", [(13, 1), (2056, 2), (4104, 2), (8200, 2)])
def test_every_tree_shape_matches_the_contract(gpu_lib, M, T):
    """256 x 8 (13 nodes padded to 16), 512 x 8, 1024 x 8 and 1024 x 16 (8200 nodes pad to 8208), with a limit mask, an
    output mask, three classes and an EV part; the drop equals revs_net_headroom's in bytes."""
    from revs_admm_amd.feeder import feeder_tree, headroom_aux, tree_report_host
    from revs_admm_amd.headroom import report_for_tree as headroom_report
    pick = np.random.default_rng(1000 + M)
    limit_nodes = np.flatnonzero(pick.random(M) < 0.6)
    nodes = np.flatnonzero(pick.random(M) < 0.7)
    classes = pick.integers(0, 3, M)
    # An excess of 2e-5 in the even slots: with hundreds of nodes sharing a drop of 0.0975, a node's own EV part clears
    # that much at some nodes and not at others.  frac = 1 / M: about the mean share, so n_big splits the nodes too.
    par, er, cons, p, ev, rng = forest_case(M, T, seed=M, peaks=(0.0975 + 2e-5, 0.09), limit_nodes=limit_nodes)
    frac = 1.0 / M
    kw = dict(limit_nodes=limit_nodes, nodes=nodes, classes=classes, frac=frac)
    if M > 2000:                                          # the inputs first, with the restatement on the CPU alone
        tree = feeder_tree(par, er, cons, np.ones(M, bool))
        rows = lambda a: np.where((tree["src"] >= 0)[:, None], a[np.maximum(tree["src"], 0)], 0.0)
        mk = lambda sel: ar.to_pos(tree, np.isin(np.arange(M), sel), False)
        host = ar.contract(tree, headroom_aux(tree), M, rows(p), rows(ev), ar.to_pos(tree, tree_report_host(tree, p, M)[1]),
                           1.0 - 0.95 ** 2, frac, limit=mk(limit_nodes), out_mask=mk(nodes))["slot"]
        assert ((host["excess"] > 0) & (host["n_can"] > 0) & (host["n_can"] < host["n_reach"])).any(), host
        assert ((host["n_big"] > 0) & (host["n_big"] < host["n_reach"])).all(), host
    rep = run(par, er, cons, p, ev, **kw)
    s = rep.slot
    print(f"M={M}: watch {s['watch']}, excess {s['excess']}, n_reach {s['n_reach']}, n_big {s['n_big']}, n_can {s['n_can']}")
    assert M < 2000 or ((s["excess"] > 0) & (s["n_can"] > 0) & (s["n_can"] < s["n_reach"])).any()
    assert (s["watch"] >= 0).all() and np.isin(s["watch"], limit_nodes).all()
    assert rep.drop.tobytes() == headroom_report(par, er, cons, p, need=0.0).drop.tobytes()
    assert (np.abs(s["total"] - s["drop_watch"]) <= 1e-12 * np.abs(rep.drop).max()).all()


def chain(n, r=1.0):
    return np.arange(-1, n - 1), np.full(n, r), np.arange(n)


def test_hand_cases(gpu_lib):
    """The host test's hand cases at T = 3 (three load levels)."""
    lv = np.array([[0.5, 1.0, 2.0]])
    run(*chain(8, 0.5), np.ones((8, 1)) / 64 * lv, vset=2.0, vmin=1.0)
    rep = run(np.full(6, -1), np.ones(6), np.arange(6), np.arange(1.0, 7.0)[:, None] / 32 * lv)
    assert (rep.slot["watch"] == 5).all() and (rep.slot["n_reach"] == 1).all()
    p5 = np.array([[1.0], [1.0], [1.0], [1.0], [3.0]]) / 64 * lv
    rep = run(np.array([-1, 0, 0, -1, 3]), np.ones(5), np.arange(5), p5, p5 * 0.5)
    assert (rep.slot["watch"] == 4).all() and rep.sens[:3].tobytes() == np.zeros((3, 3)).tobytes()
    # a tie of two limit nodes on drop, a fixed watch, no candidate at all
    par, er, cons = np.array([-1, 0, 0]), np.array([1.0, 0.5, 0.5]), np.arange(3)
    p3 = np.array([[0.0], [0.25], [0.25]]) * lv
    assert (run(par, er, cons, p3).slot["watch"] == 1).all()
    assert (run(par, er, cons, p3, watch=0).slot["watch"] == 0).all()
    rep = run(par, er, cons, p3, p3, limit_nodes=[])
    assert (rep.slot["watch"] == -1).all() and not rep.sens.any() and (rep.summary["count"] == 0).all()
    assert rep.contrib.tobytes() == np.zeros((3, 3)).tobytes() and (rep.slot["n_bad"] == 0).all()
    # ev equal to its relief exactly, from powers of two: it counts; one ulp short does not
    par, er, cons = chain(4, 0.5)
    p4 = np.array([[0.0], [0.0], [0.0], [1.0]])
    ev = np.array([[1.0], [0.5], [0.5], [0.5]])
    for vset, vmin in ((2.0, np.sqrt(2.0)), (1.5, 0.5)):          # drop_max 2 (to rounding) and exactly 2
        rep = run(par, er, cons, p4, ev, vset=vset, vmin=vmin)
    assert rep.slot["excess"][0] == 2.0 and rep.slot["n_can"][0] == 1 and rep.relief()[3, 0] == 0.5
    ev[3, 0] = np.nextafter(0.5, 0.0)
    assert run(par, er, cons, p4, ev, vset=1.5, vmin=0.5).slot["n_can"][0] == 0
    assert run(par, er, cons, p4, ev, vset=3.0, vmin=0.5).slot["n_can"][0] == 0       # excess = 0: every relief 0


def test_chain_of_depth_2048(gpu_lib):
    """One lateral of 2048 nodes, the last node watched: sens[i] = wc[i] for every i.  The launch runs in a child process
    with its own time limit."""
    code = ("import numpy as np, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from revs_admm_amd.attribution import report_for_tree\n"
            "n = 2048; rng = np.random.default_rng(4)\n"
            "p = rng.uniform(0.0, 1.0, (n, 1)); p *= 0.11 / (2.0 * np.cumsum(np.cumsum(p[::-1, 0])[::-1] * 1e-3)).max()\n"
            "ev = p * rng.uniform(0.0, 1.0, p.shape)\n"
            "rep = report_for_tree(np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n), p, ev, watch=n - 1)\n"
            "np.savez(sys.argv[1], p=p, ev=ev, sens=rep.sens, contrib=rep.contrib, ev_contrib=rep.ev_contrib, drop=rep.drop,\n"
            "         slot=rep.slot.view(np.uint8), summary=rep.summary.view(np.uint8), day=rep.day.view(np.uint8))\n"
            % (HERE, os.path.dirname(HERE)))
    import tempfile
    from revs_admm_amd._lib import ATTR_DAY_DTYPE, ATTR_SLOT_DTYPE
    from revs_admm_amd.attribution import AttributionReport
    from revs_admm_amd.feeder import feeder_tree, headroom_aux
    from revs_admm_amd.network import SUMMARY_DTYPE
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "chain.npz")
        r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        g = np.load(out)
        rep = AttributionReport(g["sens"], g["contrib"], g["ev_contrib"], g["drop"], g["slot"].view(ATTR_SLOT_DTYPE),
                                g["summary"].view(SUMMARY_DTYPE), g["day"].view(ATTR_DAY_DTYPE), 0.01, 1.0, 0.95)
        p, ev = g["p"], g["ev"]
    n = 2048
    par, er, cons = np.arange(-1, n - 1), np.full(n, 1e-3), np.arange(n)
    check_report(rep, par, er, cons, p, ev, watch=n - 1)
    wc = headroom_aux(feeder_tree(par, er, cons, np.ones(n, bool)))["wc"]
    assert rep.sens[:, 0].tobytes() == wc.tobytes() and rep.slot["n_reach"][0] == n and rep.slot["excess"][0] > 0


def test_scenario_grid_equals_single_calls(gpu_lib):
    """S = 3 x T = 5 on 300 nodes with masks and classes: every scenario against the contract, and its slice equal in
    bytes to the S = 1 call on that scenario."""
    from revs_admm_amd.attribution import report_for_tree
    par, er, cons, p, ev, rng = forest_case(300, 5, seed=300)
    ps = np.stack([p, p * rng.uniform(0.5, 1.1, p.shape), p[::-1].copy()])
    evs = np.stack([ev, 0.5 * ps[1], ev[::-1].copy()])
    kw = dict(limit_nodes=np.flatnonzero(rng.random(300) < 0.6), nodes=np.flatnonzero(rng.random(300) < 0.5),
              classes=rng.integers(0, 4, 300), frac=0.02)
    reps = report_for_tree(par, er, cons, ps, evs, **kw)
    assert len(reps) == 3
    for s, rep in enumerate(reps):
        check_report(rep, par, er, cons, ps[s], evs[s], **kw)
        one = report_for_tree(par, er, cons, ps[s], evs[s], **kw)
        for k in ("sens", "contrib", "ev_contrib", "drop", "slot", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (s, k)
    assert reps[0].slot["n_big"].max() > 0 and (reps[0].slot["top_index"][:, 0] >= 0).all()


def test_every_output_alone_and_records_only(gpu_lib):
    """Each output with every other one NULL holds the bytes of the full call; arrays=False gives the same records."""
    import ctypes as C
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.attribution import class_array, report_for_tree
    from revs_admm_amd.headroom import aux_on_device, position_mask
    from revs_admm_amd.network import SUMMARY_DTYPE, side_arrays, tree_on_device
    par, er, cons, p, ev, rng = forest_case(300, 4, seed=12)
    classes = rng.integers(0, 3, 300)
    full = report_for_tree(par, er, cons, p, ev, classes=classes)
    only = report_for_tree(par, er, cons, p, ev, classes=classes, arrays=False)
    assert only.sens is None and only.contrib is None and only.ev_contrib is None and only.drop is None
    for k in ("slot", "summary", "day"):
        assert getattr(only, k).tobytes() == getattr(full, k).tobytes(), k
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    aux, _k2 = aux_on_device(dev, th)
    d_nop = side_arrays(dev, th, 300, None, None)[0]
    d_outm = position_mask(dev, th, 300, None)
    d_cls, n_cls = class_array(dev, th, 300, classes)
    g, e = torch.from_numpy(p).to(dev), torch.from_numpy(ev).to(dev)
    scratch = torch.empty(lib.revs_net_attribution_scratch(1, 4, th["n"]) // 8 + 1, dtype=torch.float64, device=dev)
    wants = [full.sens, full.contrib, full.ev_contrib, full.drop, full.slot, full.summary, full.day]
    sizes = [300 * 4 * 8] * 4 + [4 * _lib.ATTR_SLOT_DTYPE.itemsize, 4 * SUMMARY_DTYPE.itemsize, 300 * _lib.ATTR_DAY_DTYPE.itemsize]
    for k in range(7):
        outs = [None] * 7
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = lib.revs_net_attribution(1, 300, 4, C.byref(tree), C.byref(aux), g.data_ptr(), e.data_ptr(), None,
                                      d_outm.data_ptr(), d_cls.data_ptr(), n_cls, d_nop.data_ptr(), 300, -1,
                                      1.0 - 0.95 ** 2, 0.01, *[None if o is None else o.data_ptr() for o in outs],
                                      scratch.data_ptr() if k >= 4 else None, None)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k


def test_bad_slots(gpu_lib):
    """A NaN / inf in one slot of three, in node_g and separately in node_ev: that slot reads NaN / -1 / n_bad 1, the others
    keep their bytes.  Without node_ev: ev_total +0.0, n_can 0."""
    par, er, cons, p, ev, rng = forest_case(300, 3, seed=7)
    clean = run(par, er, cons, p, ev)
    for which in ("g", "ev"):
        for bad in (np.nan, np.inf):
            q, qe = p.copy(), ev.copy()
            (q if which == "g" else qe)[17, 1] = bad
            rep = run(par, er, cons, q, qe)
            assert np.isnan(rep.sens[:, 1]).all() and np.isnan(rep.contrib[:, 1]).all() and np.isnan(rep.ev_contrib[:, 1]).all()
            s = rep.slot[1]
            assert s["watch"] == -1 and s["n_bad"] == 1 and s["n_reach"] == s["n_big"] == s["n_can"] == 0
            assert np.isnan([s["drop_watch"], s["excess"], s["total"], s["ev_total"]]).all() and np.isnan(s["class_total"]).all()
            assert np.isnan(s["top_value"]).all() and (s["top_index"] == -1).all()
            assert rep.summary["count"][1] == 0 and rep.summary["n_nan"][1] == 300
            for k in ("sens", "contrib", "ev_contrib", "drop"):
                assert getattr(rep, k)[:, [0, 2]].tobytes() == getattr(clean, k)[:, [0, 2]].tobytes(), k
            assert rep.slot[[0, 2]].tobytes() == clean.slot[[0, 2]].tobytes()
            assert rep.summary[[0, 2]].tobytes() == clean.summary[[0, 2]].tobytes()
            assert (rep.day["peak_slot"] != 1).all() and not np.isnan(rep.day["peak"]).any()
    rep = run(par, er, cons, np.full_like(p, np.nan), ev)
    assert np.isnan(rep.day["peak"]).all() and (rep.day["peak_slot"] == -1).all() and not rep.day["sum"].any()
    rep = run(par, er, cons, p)
    assert rep.ev_contrib is None and rep.slot["ev_total"].tobytes() == np.zeros(3).tobytes() and (rep.slot["n_can"] == 0).all()
    assert rep.slot["total"].tobytes() == clean.slot["total"].tobytes() and rep.sens.tobytes() == clean.sens.tobytes()


def _small_workload():
    from helpers import f32
    from revs_admm_amd.synthetic import make_workload
    w = make_workload(2000, 24, n_nodes=64, seed=3, binary_feasible=False)
    w.load, w.cost = f32(w.load), f32(w.cost)
    return w


def test_engine_attribution_report(gpu_lib):
    """After a short streaming run: attribution_report() of the schedule and of a rule schedule against the contract; the
    EV node sums are np.add.at of P_sch; the run's state keeps its bytes."""
    from revs_admm_amd.engine import AdmmEngine
    w = _small_workload()
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                   mode="pdhg", feeder=w.feeder)
    e.run(3)
    e.run_steps(10)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    classes = np.arange(w.M) % 4
    rep = e.attribution_report(classes=classes)
    assert (rep.vset, rep.vmin) == (w.vset, w.vlow)
    has = np.flatnonzero(np.bincount(w.node_of, minlength=w.M) > 0)
    sch = e.result()[0].astype(np.float64)
    g, ev = np.zeros((w.M, 24)), np.zeros((w.M, 24))
    np.add.at(g, w.node_of, w.load.astype(np.float64) + sch)
    np.add.at(ev, w.node_of, sch)
    kw = dict(limit_nodes=has, nodes=has, vset=w.vset, vmin=w.vlow)
    check_report(rep, w.parent, w.edge_r, np.arange(w.M), g, ev, classes=classes, **kw)
    prof = e.rule_schedule("uncontrolled")
    rule = e.attribution_report(profile=prof, watch=int(has[-1]), frac=0.05)
    prof_h = prof if isinstance(prof, np.ndarray) else prof.cpu().numpy()[e.inv_perm]
    g2, ev2 = np.zeros((w.M, 24)), np.zeros((w.M, 24))
    np.add.at(g2, w.node_of, prof_h.astype(np.float64))
    np.add.at(ev2, w.node_of, (prof_h.astype(np.float32) - w.load.astype(np.float32)).astype(np.float64))   # (formed in float32)
    check_report(rule, w.parent, w.edge_r, np.arange(w.M), g2, ev2, watch=int(has[-1]), frac=0.05, **kw)
    assert (rule.slot["watch"] == has[-1]).all()
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    e.run_steps(2)


def test_ensemble_attribution_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.attribution_reports()[s] holds the bytes of a single engine's report on scenario s."""
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    classes = np.arange(w.M) % 2
    reps = ens.attribution_reports(classes=classes, frac=0.02)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.attribution_report(classes=classes, frac=0.02)
        for k in ("sens", "contrib", "ev_contrib", "drop", "slot", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)


SHARD_CASE = dict(name="attr", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports --
    of the schedule after 4 iterations, and of a given profile with a fixed watch -- hold the one-rank bytes."""
    sys.path.insert(0, HERE)
    from attribution_worker import reports
    from network_worker import engine
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_contrib"]).all() and ref["sch_sens"].any()
    port = 31900 + os.getpid() % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "attribution_worker.py"), str(path)], stdout=log,
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
        got = np.load(tmp_path / f"attr_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


def test_study_fills_attribution(gpu_lib, golden):
    """REVS.study(attribution=True) on the 121144 feeder, 2 seeds x {individual, uncontrolled}: StudyReport.attribution[s]
    holds the bytes of report_for_tree on the report's own row s with the EV part = that row minus the base load,
    summarised over the community; the default leaves it None."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.attribution import report_for_tree
    from revs_admm_amd.lpsolver import feeder_of
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), methods=("individual", "uncontrolled"), arrays=True)
    labels, rep = REVS().study(tariff, all_homes, dist, com, attribution=True, **grid)
    assert REVS().study(tariff, all_homes, dist, com, **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].attribution is None
    assert len(rep.attribution) == len(labels) == 4
    parent, edge_r, cons_of = feeder_of(dist)[1]
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    pos = {n: i for i, n in enumerate(nonsub)}
    nodes = [pos[h] for h in com]
    base = np.array([all_homes[h] for h in res], np.float64)
    for s, got in enumerate(rep.attribution):
        one = report_for_tree(parent, edge_r, cons_of, rep.node_p[s], rep.node_p[s] - base, nodes=nodes)
        for k in ("sens", "contrib", "ev_contrib", "drop", "slot", "summary", "day"):
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert (got.slot["n_bad"] == 0).all() and (got.slot["watch"] >= 0).all()
