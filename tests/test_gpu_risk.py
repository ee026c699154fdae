"""The risk report on the GPU (revs_net_risk; risk.report_for_tree, AdmmEngine.risk_report, AdmmEnsemble.risk_reports,
REVS.study(risk=...)) against tests/risk_ref.py: drop equal to revs_net_headroom's in bytes; sd against the restated
variance within BOUND x max(var); bit for bit the contract fed the kernel's own sd and drop -- z, drop_q, the slot records,
the day records, the summary's order statistics and counts (the interpolated quartiles within 2 ulp) --; expected and
expected_slots bit for bit the fixed-tree and slot-order sums of the kernel's own prob; prob within PROB_ULPS of libm's
erfc on the kernel's own z; every tree shape and the code paths behind them."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import risk_ref as rr
from test_gpu_network import BOUND, golden_net, synthetic_forest  # noqa: F401  (golden_net: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLOT_FIELDS = ("expected", "z_min", "sd_at", "drop_at", "sd_max", "n_risky", "n_det", "z_min_index", "n_bad")
DAY_FIELDS = ("prob_max", "z_min", "expected_slots", "prob_max_slot", "n_risky")
ARRAYS = ("sd", "z", "prob", "drop_q", "drop")
# prob against 0.5 math.erfc(z 0.7071067811865476) on the kernel's own z, in ulps of prob.  The device library's erfc and
# libm's are different implementations, each claiming a few ulp.  The largest deviation over this file's cases, measured
# on the MI355X, is 3 ulp (at probs from 1e-2 down to 1e-197); the bound is twice that, rounded up
# to a power of two.
PROB_ULPS = 8
worst_prob_ulps = [0.0]


def same(a, b):
    """Equal in bytes, NaNs at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == b[~nan].tobytes()


def restate(par, er, cons, p, var, com, limit_nodes, nodes):
    """The host side of a case by position: (tree, var restated by risk_ref.path_form, limit mask, output mask, bad)."""
    from revs_admm_amd.feeder import feeder_tree, headroom_aux, risk_weights
    n = len(par)
    tree = feeder_tree(par, er, cons, np.ones(p.shape[0], bool))
    rows = lambda a: np.where((tree["src"] >= 0)[:, None], a[np.maximum(tree["src"], 0)], 0.0)
    T = p.shape[1]
    s2 = np.zeros((tree["n"], T)) if var is None else rows(var)
    betas = [] if com is None else [rows(b) for b in com]
    bad = ~np.isfinite(rows(p)).all(axis=0) | ~np.isfinite(s2).all(axis=0) | (s2 < 0.0).any(axis=0)
    for b in betas:
        bad |= ~np.isfinite(b).all(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        var_ref, _ = rr.path_form(tree, risk_weights(tree, headroom_aux(tree)), s2, betas)

    def mask(sel):                                       # None: the nodes that carry a row, the report's default
        mk = np.zeros(n, bool)
        if sel is None:
            mk[:] = np.asarray(cons) >= 0
        else:
            mk[np.asarray(sel, np.int64)] = True
        return rr.to_pos(tree, mk, False)

    return tree, var_ref, None if limit_nodes is None else mask(limit_nodes), mask(nodes), bad


def check_prob(prob, z):
    """prob against libm's erfc on the kernel's own z: PROB_ULPS ulp of prob; below 1e-300 absolutely against 1e-300."""
    ok = ~np.isnan(z)
    assert np.array_equal(np.isnan(prob), ~ok)
    want = np.array([0.5 * math.erfc(v * rr.INV_SQRT2) for v in z[ok]])
    got = prob[ok]
    tiny = want < 1e-300
    assert (np.abs(got[tiny] - want[tiny]) <= 1e-300).all()
    u = np.abs(got[~tiny] - want[~tiny]) / np.spacing(want[~tiny])
    if u.size:
        worst_prob_ulps[0] = max(worst_prob_ulps[0], float(u.max()))
        at = int(np.argmax(u))
        print(f"prob against libm: worst {u.max():.2f} ulp at prob = {want[~tiny][at]:.3e}, z = {z[ok][~tiny][at]:.4f}; "
              f"so far {worst_prob_ulps[0]:.2f}")
        assert u.max() <= PROB_ULPS, (u.max(), want[~tiny][at])
    inf = np.isinf(z[ok])
    assert (got[inf] == np.where(z[ok][inf] > 0, 0.0, 1.0)).all()


def check_report(rep, par, er, cons, p, var=None, com=None, limit_nodes=None, nodes=None, vset=1.0, vmin=0.95, p_max=0.05):
    from revs_admm_amd.risk import z_of
    n = len(par)
    tree, var_ref, lim, om, bad = restate(par, er, cons, p, var, com, limit_nodes, nodes)
    z_max, drop_max = z_of(p_max), vset * vset - vmin * vmin
    assert (rep.z_max, rep.p_max, rep.vset, rep.vmin) == (z_max, p_max, vset, vmin)
    sd, drop, prob = (rr.to_pos(tree, getattr(rep, k)) for k in ("sd", "drop", "prob"))
    good = ~bad
    if good.any():
        gap = np.abs(sd[:, good] ** 2 - var_ref[:, good]).max()
        print(f"sd^2 against the restated variance: {gap:.3e} (bound {BOUND * var_ref[:, good].max():.3e})")
        assert gap <= BOUND * var_ref[:, good].max()
    assert np.isnan(rep.sd[:, bad]).all() and (rep.sd[:, good] >= 0.0).all()
    out = rr.contract(tree, n, np.where(np.isnan(sd), 0.0, sd), drop, drop_max, z_max, limit=lim, out_mask=om, bad=bad,
                      prob=prob)
    for k in ("z", "drop_q"):
        want = rr.to_nodes(tree, out[k], n)
        assert same(getattr(rep, k), want), (k, np.nanmax(np.abs(getattr(rep, k) - want)))
    for k in SLOT_FIELDS:
        assert same(rep.slot[k], out["slot"][k]), (k, rep.slot[k], out["slot"][k])
    assert not rep.slot["reserved"].any()
    rr.check_summary(rep.summary, out["summary"])
    for k in DAY_FIELDS:
        assert same(rep.day[k], out["day"][k]), (k, np.flatnonzero(rep.day[k] != out["day"][k])[:5])
    check_prob(rep.prob, rep.z)
    with np.errstate(invalid="ignore"):
        assert same(rep.voltage_q(), np.sqrt(vset * vset - rep.drop_q))
    assert same(rep.prob_any(), 1.0 - np.prod(np.where(np.isnan(rep.prob), 1.0, 1.0 - rep.prob), axis=1))
    return out


def run(par, er, cons, p, var=None, com=None, **kw):
    from revs_admm_amd.risk import report_for_tree
    rep = report_for_tree(par, er, cons, p, var, None if com is None else np.stack(com), **kw)
    check_report(rep, par, er, cons, p, var, com, **kw)
    return rep


def forest_case(M, T, seed, peaks=(0.095, 0.085), limit_nodes=None):
    """A forest of M nodes, every node a row, loads scaled slot by slot as test_gpu_attribution.forest_case scales them --
    the deepest drop among the limit nodes in slot t is peaks[t % 2] against drop_max = 0.0975 --, independent errors of
    10 % of every row's load and two shared factors that move the loads by 5 % and by a random 0 .. 4 %: the deepest
    node's sd is about 0.006, so it sits within about half an sd of the limit in the even slots and two in the odd ones."""
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed)
    p = rng.uniform(0.0, 4.0, (M, T))
    _, drop = tree_report_host(feeder_tree(par, er, cons, np.ones(M, bool)), p, M)
    top = (drop if limit_nodes is None else drop[limit_nodes]).max(axis=0)
    p = p * (np.array([peaks[t % 2] for t in range(T)]) / top)[None, :]
    return par, er, cons, p, (0.1 * p) ** 2, [0.05 * p, p * rng.uniform(0.0, 0.04, p.shape)], rng


@pytest.mark.parametrize("M,T", [(13, 1), (2056, 2), (4104, 2), (8200, 2)])
def test_every_tree_shape_matches_the_contract(gpu_lib, M, T):
    """256 x 8 (13 nodes padded to 16), 512 x 8, 1024 x 8 and 1024 x 16 (8200 nodes pad to 8208), with a limit mask, an
    output mask, node_var and K = 2; the drop equals revs_net_headroom's in bytes."""
    from revs_admm_amd.feeder import tree_report_host
    from revs_admm_amd.headroom import report_for_tree as headroom_report
    from revs_admm_amd.risk import z_of
    pick = np.random.default_rng(1000 + M)
    limit_nodes = np.flatnonzero(pick.random(M) < 0.6)
    nodes = np.flatnonzero(pick.random(M) < 0.7)
    par, er, cons, p, var, com, rng = forest_case(M, T, seed=M, limit_nodes=limit_nodes)
    kw = dict(limit_nodes=limit_nodes, nodes=nodes)
    # the inputs first, with the restatement on the CPU alone: the counts must split the covered nodes in some slot
    tree, var_ref, lim, om, bad = restate(par, er, cons, p, var, com, limit_nodes, nodes)
    drop = rr.to_pos(tree, tree_report_host(tree, p, M)[1])
    host = rr.contract(tree, M, np.sqrt(var_ref), drop, 1.0 - 0.95 ** 2, z_of(0.05), limit=lim, out_mask=om)
    count = int(host["cov"].sum())
    assert ((host["slot"]["n_risky"] > 0) & (host["slot"]["n_risky"] < count)).any(), (host["slot"]["n_risky"], count)
    assert not bad.any() and (host["slot"]["n_det"] == 0).all() and (host["slot"]["z_min"] < 1.0).any()
    rep = run(par, er, cons, p, var, com, **kw)
    s = rep.slot
    print(f"M={M}: covered {count}, n_risky {s['n_risky']}, n_det {s['n_det']}, z_min {s['z_min']} at {s['z_min_index']}, "
          f"expected {s['expected']}, sd_max {s['sd_max']}")
    assert ((s["n_risky"] > 0) & (s["n_risky"] < count)).any() and np.array_equal(s["n_risky"], host["slot"]["n_risky"])
    assert np.isin(s["z_min_index"], np.intersect1d(limit_nodes, nodes)).all()
    assert rep.drop.tobytes() == headroom_report(par, er, cons, p, need=0.0).drop.tobytes()


def chain(n, r=1.0):
    return np.arange(-1, n - 1), np.full(n, r), np.arange(n)


def test_no_variance_is_the_deterministic_report(gpu_lib):
    """node_var = NULL and K = 0 on the 13-node forest: sd = 0, z = +-inf by the sign of the slack, prob 0 or 1, and
    n_risky == n_det.  A slack of exactly 0 with sd = 0: z = +inf."""
    par, er, cons, p, _, _, _ = forest_case(13, 2, seed=13, peaks=(0.11, 0.09))
    rep = run(par, er, cons, p)
    assert not rep.sd.any() and np.isinf(rep.z).all() and np.isin(rep.prob, (0.0, 1.0)).all()
    assert np.array_equal(rep.z > 0, rep.drop <= rep.drop_max) and np.array_equal(rep.prob == 1.0, rep.drop > rep.drop_max)
    assert np.array_equal(rep.slot["n_risky"], rep.slot["n_det"]) and rep.slot["n_det"][0] > 0 and rep.slot["n_det"][1] == 0
    assert rep.drop_q.tobytes() == rep.drop.tobytes()
    # chain of 4, r = 0.5 (w = 1), load 1 at the end: drop = 1, 2, 3, 4; drop_max = 1.5^2 - 0.5^2 = 2 exactly
    rep = run(*chain(4, 0.5), np.array([[0.0], [0.0], [0.0], [1.0]]), vset=1.5, vmin=0.5)
    assert rep.drop[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and rep.drop_max == 2.0
    assert rep.z[:, 0].tolist() == [np.inf, np.inf, -np.inf, -np.inf] and rep.prob[:, 0].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert rep.slot["n_risky"][0] == rep.slot["n_det"][0] == 2 and rep.slot["z_min_index"][0] == 2
    assert rep.slot["expected"][0] == 2.0 and rep.day["n_risky"].tolist() == [0, 0, 1, 1]
    # the same chain with a variance at the last row alone: sd = wc[lca] sqrt(s2) = 1, 2, 3, 4 times 0.5
    rep = run(*chain(4, 0.5), np.array([[0.0], [0.0], [0.0], [1.0]]), np.array([[0.0], [0.0], [0.0], [0.25]]),
              vset=1.5, vmin=0.5)
    assert rep.sd[:, 0].tolist() == [0.5, 1.0, 1.5, 2.0] and rep.z[:, 0].tolist() == [2.0, 0.0, -1.0 / 1.5, -1.0]
    assert rep.prob[1, 0] == 0.5


def test_bad_slots(gpu_lib):
    """A NaN in node_var, a negative variance, an inf in a loading and a NaN in node_g, each in one slot of two on the
    13-node forest: that slot reads NaN / -1 / n_bad 1 with the counts 0, the other keeps its bytes."""
    par, er, cons, p, var, com, rng = forest_case(13, 2, seed=13)
    clean = run(par, er, cons, p, var, com)
    for which, bad in (("var", np.nan), ("var", -1e-9), ("com", np.inf), ("g", np.nan)):
        q, qv, qc = p.copy(), var.copy(), [c.copy() for c in com]
        dict(g=q, var=qv, com=qc[1])[which][5, 1] = bad
        rep = run(par, er, cons, q, qv, qc)
        for k in ("sd", "z", "prob", "drop_q"):
            assert np.isnan(getattr(rep, k)[:, 1]).all(), (which, k)
        s = rep.slot[1]
        assert s["n_bad"] == 1 and s["n_risky"] == s["n_det"] == 0 and s["z_min_index"] == -1
        assert np.isnan([s["expected"], s["z_min"], s["sd_at"], s["drop_at"], s["sd_max"]]).all()
        assert rep.summary["count"][1] == 0 and rep.summary["n_nan"][1] == 13
        for k in ARRAYS:
            assert getattr(rep, k)[:, 0].tobytes() == getattr(clean, k)[:, 0].tobytes(), (which, k)
        assert rep.slot[0].tobytes() == clean.slot[0].tobytes() and rep.summary[0].tobytes() == clean.summary[0].tobytes()
        if which != "g":
            assert rep.drop.tobytes() == clean.drop.tobytes()          # (drop_out stays what the scans give)
        assert (rep.day["prob_max_slot"] == 0).all() and not np.isnan(rep.day["prob_max"]).any()
    rep = run(par, er, cons, p, np.full_like(var, np.nan), com)
    assert np.isnan(rep.day["prob_max"]).all() and (rep.day["prob_max_slot"] == -1).all() and not rep.day["expected_slots"].any()


def test_scenario_grid_equals_single_calls(gpu_lib):
    """S = 3 x T = 2 on the 13-node forest and on 300 nodes with masks: every scenario against the contract, and its slice
    equal in bytes to the S = 1 call on that scenario."""
    from revs_admm_amd.risk import report_for_tree
    for M in (13, 300):
        par, er, cons, p, var, com, rng = forest_case(M, 2, seed=M)
        ps = np.stack([p, p * rng.uniform(0.5, 1.1, p.shape), p[::-1].copy()])
        vs = np.stack([var, 0.25 * var, var[::-1].copy()])
        cs = np.stack([np.stack([c, 0.5 * c, c[::-1].copy()]) for c in com])           # (K, S, M, T)
        kw = dict(limit_nodes=np.flatnonzero(rng.random(M) < 0.6), nodes=np.flatnonzero(rng.random(M) < 0.7), p_max=0.1)
        reps = report_for_tree(par, er, cons, ps, vs, cs, **kw)
        assert len(reps) == 3
        for s, rep in enumerate(reps):
            check_report(rep, par, er, cons, ps[s], vs[s], list(cs[:, s]), **kw)
            one = report_for_tree(par, er, cons, ps[s], vs[s], np.ascontiguousarray(cs[:, s]), **kw)
            for k in ARRAYS + ("slot", "summary", "day"):
                assert getattr(one, k).tobytes() == getattr(rep, k).tobytes(), (M, s, k)


def test_every_output_alone_and_records_only(gpu_lib):
    """Each output with every other one NULL holds the bytes of the full call; arrays=False gives the same records."""
    import ctypes as C
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.feeder import risk_weights
    from revs_admm_amd.headroom import aux_on_device, position_mask
    from revs_admm_amd.network import SUMMARY_DTYPE, side_arrays, tree_on_device
    from revs_admm_amd.risk import report_for_tree, z_of
    par, er, cons, p, var, com, rng = forest_case(300, 4, seed=12)
    full = report_for_tree(par, er, cons, p, var, np.stack(com))
    only = report_for_tree(par, er, cons, p, var, np.stack(com), arrays=False)
    assert all(getattr(only, k) is None for k in ARRAYS)
    for k in ("slot", "summary", "day"):
        assert getattr(only, k).tobytes() == getattr(full, k).tobytes(), k
    lib, dev = gpu_lib, torch.device("cuda:0")
    th, tree, _k = tree_on_device(dev, par, er, cons, 300)
    aux, _k2 = aux_on_device(dev, th)
    d_nop = side_arrays(dev, th, 300, None, None)[0]
    d_outm = position_mask(dev, th, 300, None)
    d_w2 = torch.from_numpy(risk_weights(th)).to(dev)
    g, v, c = torch.from_numpy(p).to(dev), torch.from_numpy(var).to(dev), torch.from_numpy(np.stack(com)[:, None].copy()).to(dev)
    scratch = torch.empty(lib.revs_net_risk_scratch(1, 4, th["n"]) // 8 + 1, dtype=torch.float64, device=dev)
    wants = [getattr(full, k) for k in ARRAYS] + [full.slot, full.summary, full.day]
    sizes = [300 * 4 * 8] * 5 + [4 * _lib.RISK_SLOT_DTYPE.itemsize, 4 * SUMMARY_DTYPE.itemsize, 300 * _lib.RISK_DAY_DTYPE.itemsize]
    for k in range(8):
        outs = [None] * 8
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = lib.revs_net_risk(1, 300, 4, C.byref(tree), C.byref(aux), g.data_ptr(), v.data_ptr(), c.data_ptr(), 2,
                               d_w2.data_ptr(), None, d_outm.data_ptr(), d_nop.data_ptr(), 300, 1.0 - 0.95 ** 2, z_of(0.05),
                               *[None if o is None else o.data_ptr() for o in outs], scratch.data_ptr() if k >= 6 else None,
                               None)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k


def _same_reports(a, b, what):
    for k in ARRAYS + ("slot", "summary", "day"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


def test_engine_risk_report_on_the_golden_feeder(gpu_lib, golden, golden_net, feeder_R):
    """After 3 iterations on the 121144 feeder: risk_report() holds the bytes of risk_report_device on the engine's own
    node sums; rel_sd = 0 reproduces the network report's undervoltage counts in n_det, and n_risky equals them; the
    run's state keeps its bytes."""
    import torch
    from conftest import golden_homes
    from helpers import f32
    from revs_admm_amd.engine import AdmmEngine, pack_homes
    from revs_admm_amd.network import profile_node_sums
    from revs_admm_amd.risk import risk_report_device
    z, gn = golden[0], golden_net
    oh, evi = golden_homes(z, "dis_a90_r4800", 4.8)
    n, T = oh.LOAD.shape
    e = AdmmEngine(f32(z["tariff_shift6"]), pack_homes(oh.ev, 4.8, 20.0, 0.2, 11, 23), f32(oh.LOAD), np.arange(n),
                   feeder_R, kappa=5.0, vset=1.03, vlow=0.95, vhigh=1.05, mode="binary", feeder=gn["feeder"])
    e.run(3)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    rep = e.risk_report(rel_sd=0.1, ev_rel_sd=0.2, common=[("load", 0.05), ("ev", 0.1)])
    who = "test"
    sd = 0.1 * e.load + 0.2 * e.P_sch
    var = profile_node_sums(e, (sd * sd).contiguous(), who)
    com = torch.stack([profile_node_sums(e, (0.05 * e.load).contiguous(), who),
                       profile_node_sums(e, (0.1 * e.P_sch).contiguous(), who)])
    one = risk_report_device(profile_node_sums(e, None, who), var, com, tree=(e._tree, e._tree_host, e._tree_nodes),
                             vset=1.03, vmin=0.95, lib=e.lib, stream=e.stream)
    _same_reports(rep, one, "engine")
    assert (rep.slot["n_bad"] == 0).all() and (rep.slot["sd_max"] > 0).all()
    assert (rep.slot["n_risky"] >= rep.slot["n_det"]).all() and (rep.slot["n_risky"] > rep.slot["n_det"]).any()
    det = e.risk_report(rel_sd=0.0)
    net = e.network_report(nodes=gn["rows"])
    print("n_det", det.slot["n_det"], "\nn_risky at rel_sd 0.1", rep.slot["n_risky"])
    assert np.array_equal(det.slot["n_det"], net.summary_volt["n_violations"]) and det.slot["n_det"].any()
    assert np.array_equal(det.slot["n_risky"], det.slot["n_det"]) and np.array_equal(rep.slot["n_det"], det.slot["n_det"])
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    with pytest.raises(ValueError, match="p_max must lie in"):
        e.risk_report(p_max=0.0)


def test_ensemble_risk_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.risk_reports()[s] for S = 2 holds the bytes of a single engine's report on scenario s, and of
    risk_report_device on that scenario's slices of the ensemble's own node sums."""
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.risk import risk_report_device
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(2)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    opts = dict(rel_sd=0.15, ev_rel_sd=0.3, common=[("ev", 0.2), ("load", 0.05)], p_max=0.02)
    reps = ens.risk_reports(**opts)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes() and len(reps) == 2
    node_g = ens.node_sums(None, True)
    ld = ens.load.view(ens.P_sch.shape)
    sd = 0.15 * ld + 0.3 * ens.P_sch
    node_var = ens.node_sums((sd * sd).contiguous(), False)
    com = [ens.node_sums((0.2 * ens.P_sch).contiguous(), False), ens.node_sums((0.05 * ld).contiguous(), False)]
    for s in range(2):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        _same_reports(e.risk_report(**opts), reps[s], ("engine", s))
        one = risk_report_device(node_g[s].contiguous(), node_var[s].contiguous(),
                                 __import__("torch").stack([c[s] for c in com]).contiguous(),
                                 tree=ens._report_tree(), vset=w.vset, vmin=w.vlow, p_max=0.02, lib=ens.lib, stream=ens.stream)
        _same_reports(one, reps[s], ("device", s))
    assert any((r.slot["sd_max"] > 0).all() for r in reps)


SHARD_CASE = dict(name="risk", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports --
    of the schedule after 4 iterations, and of a given profile with its own standard deviations -- hold the one-rank
    bytes."""
    sys.path.insert(0, HERE)
    from network_worker import engine
    from risk_worker import reports
    from sharded_worker import make_case
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_sd"]).all() and ref["sch_sd"].any() and ref["prof_sd"].any()
    port = 33900 + os.getpid() % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "risk_worker.py"), str(path)], stdout=log,
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
        got = np.load(tmp_path / f"risk_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


def test_study_fills_risk(gpu_lib, golden):
    """REVS.study(risk=dict(rel_sd=0.1)) on the 121144 feeder, 2 seeds x {individual, uncontrolled}: StudyReport.risk[s] on
    the upload path holds the bytes of report_for_tree on the report's own row s with the variance (0.1 x the base load)^2,
    summarised over the community; the path that assembles the rows on the device gives equal records; the default leaves
    it None."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.lpsolver import feeder_of
    from revs_admm_amd.revs_fixture import REVS
    from revs_admm_amd.risk import report_for_tree
    z = golden[0]
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), methods=("individual", "uncontrolled"), arrays=True)
    labels, rep = REVS().study(tariff, all_homes, dist, com, risk=dict(rel_sd=0.1), **grid)
    assert REVS().study(tariff, all_homes, dist, com, **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].risk is None
    assert len(rep.risk) == len(labels) == 4
    _, dev_rep = REVS().study(tariff, all_homes, dist, com, risk=dict(rel_sd=0.1), ensemble=True, device_report=True, **grid)
    parent, edge_r, cons_of = feeder_of(dist)[1]
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    pos = {n: i for i, n in enumerate(nonsub)}
    nodes = [pos[h] for h in com]
    base = np.array([all_homes[h] for h in res], np.float64)
    for s, got in enumerate(rep.risk):
        one = report_for_tree(parent, edge_r, cons_of, rep.node_p[s], (0.1 * base) ** 2, nodes=nodes)
        _same_reports(one, got, ("upload", s))
        _same_reports(dev_rep.risk[s], got, ("device", s))
        assert (got.slot["n_bad"] == 0).all() and (got.slot["n_risky"] >= got.slot["n_det"]).all()
    assert any((r.slot["n_risky"] > r.slot["n_det"]).any() for r in rep.risk)
    both = REVS().study(tariff, all_homes, dist, com, risk=dict(ev_rel_sd=0.5, common=[("load", 0.05)], p_max=0.01),
                        **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].risk[0]
    assert both.p_max == 0.01 and (both.slot["sd_max"] > 0).all()
