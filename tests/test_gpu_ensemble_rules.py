"""AdmmEngine / AdmmEnsemble.rule_schedule, bill_report(baseline=<a rule>) and REVS.study with a rule method on the GPU
(revs_admm_amd/baselines.py): the net load from the records on the device is, bit for bit,
baselines.rule_schedule on every scenario's records in the caller's order; the reports take it as their profile; the bill
report's rule baseline is the uploaded array's; the run's state is left alone; the study's rule rows are the same on the
host path and on the device_report path."""
import numpy as np
import pytest

import bills_ref as br
from network_worker import line_ratings
from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
from test_gpu_ensemble_report import _mixed_ensemble, _same_report, _sequential_sums
from test_gpu_study import BANDS

pytestmark = pytest.mark.gpu

S, N, T = 5, 600, 24


def _caller_order(e, g):
    """(n, S, T) on the device in the engine's residence order -> (S, n, T) numpy in the caller's."""
    return np.ascontiguousarray(g.cpu().numpy()[e.inv_perm].transpose(1, 0, 2))


def test_ensemble_rule_schedule_and_its_reports(gpu_lib):
    import torch
    from revs_admm_amd import baselines, study
    w, load, e = _mixed_ensemble(2)
    homes = _mixed_scenarios(w, S)
    first = None
    for policy in ("uncontrolled", "last_minute", "trickle"):
        for fill in ("target", "full"):
            g = e.rule_schedule(policy, fill)
            assert tuple(g.shape) == (N, S, T) and g.dtype == torch.float32 and g.is_contiguous() and g.device == e.dev
            gc = _caller_order(e, g)
            for s in range(S):
                want = baselines.rule_schedule(homes[s], load[s], policy, fill, "continuous")[2]
                assert gc[s].tobytes() == want.tobytes(), (policy, fill, s)
            first = g if first is None else first
    # the engine's mode decides the charger (relaxed_exact: continuous); an on/off charger on the same records differs
    gb = _caller_order(e, e.rule_schedule("uncontrolled", "target", charger="binary"))
    for s in range(S):
        assert gb[s].tobytes() == baselines.rule_schedule(homes[s], load[s], "uncontrolled", "target", "binary")[2].tobytes()
    g = first
    gc = _caller_order(e, g)
    assert (gb != gc).any() and np.abs(gc[3] - gc[0]).max() > 0.1
    with pytest.raises(ValueError, match="trickle"):
        e.rule_schedule("trickle", charger="binary")
    # the reports take it as their profile: the host-upload entry fed the same node sums
    rating, nodes = line_ratings(w)
    par, er, cons = w.feeder
    groups = [0, 0, 1, 1, -1]
    rep = e.study_report(groups=groups, rating=rating, nodes=nodes, arrays=True, profile=g)
    assert rep.node_p.tobytes() == _sequential_sums(e, gc.astype(np.float64)).tobytes()
    ref = study.study_report(par, er, cons, rep.node_p, groups=groups, rating=rating, nodes=nodes, bands=BANDS,
                             vset=w.vset, vmin=w.vlow, vmax=w.vhigh, arrays=True)
    _same_report(rep, ref, arrays=True)
    v = e.voltages(profile=g).cpu().numpy()
    assert v.shape[0] == S and np.isfinite(v).all() and len(e.network_reports(rating=rating, nodes=nodes, profile=g)) == S
    # uncontrolled charging is harder on the feeder than the schedules the ADMM run left
    run = e.study_report(groups=groups, rating=rating, nodes=nodes)
    print("lowest voltage: uncontrolled", rep.summary_volt["min"].min(), "ADMM after 2 iterations", run.summary_volt["min"].min())
    # the bill report: the rule's name is the rule's net load uploaded as the baseline
    named = e.bill_report(baseline="uncontrolled", groups=groups)
    given = e.bill_report(baseline=gc.astype(np.float64), groups=groups)
    br.same_report(named, given)
    assert named.bill.shape == (2 * S, N) and named.base.tolist() == [5, 6, 7, 8, 9] + [-1] * 5
    full = e.bill_report(baseline="last_minute", groups=groups, baseline_fill="full")
    br.same_report(full, e.bill_report(baseline=_caller_order(e, e.rule_schedule("last_minute", "full")).astype(np.float64),
                                       groups=groups))
    assert (full.bill[S:] != named.bill[S:]).any()
    with pytest.raises(ValueError, match="baseline must be"):
        e.bill_report(baseline="asap")
    with pytest.raises(ValueError, match="fill must be"):
        e.bill_report(baseline="uncontrolled", baseline_fill="half")


def test_single_engine_rule_schedule(gpu_lib):
    from revs_admm_amd import baselines
    from revs_admm_amd.engine import AdmmEngine
    w = _workload()
    eng = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh,
                     mode="relaxed_exact", feeder=w.feeder)
    g = eng.rule_schedule("trickle", "full")
    assert tuple(g.shape) == (N, T)
    want = baselines.rule_schedule(w.homes, w.load, "trickle", "full", "continuous")[2]
    assert g.cpu().numpy()[eng.inv_perm].tobytes() == want.tobytes()
    rep = eng.network_report(profile=g, arrays=False)
    assert rep.node_sums.shape == (w.M, T)


def test_individual_optimum_never_costs_more_than_uncontrolled_charging(gpu_lib):
    """On/off chargers filled to 100 %: the individual optimum takes the min(nmax, W) cheapest window slots, uncontrolled
    charging the first min(nmax, W): no EV residence pays less for the latter.  The claim needs residences whose own rows
    are not empty: where nmin > nmax (no whole number of slots ends in [0.9, 1]; many of the mixed scenarios' records,
    which were drawn for continuous chargers) the rule schedule charges nothing by its contract while the individual
    mode, which has no s_T >= 0.9 row, still takes nmax slots -- those residences are held to their contract instead:
    the uncontrolled bill is the bill of the base load."""
    w, load, _ = _mixed_ensemble(1)
    homes = _mixed_scenarios(w, S)
    e = _ensemble(w, homes, "binary", load=load)
    tariff = np.asarray(w.cost, np.float32).astype(np.float64)
    assert all((0.01 * tariff.max() < 0.99 / h["capacity"].astype(np.float64)).all() for h in homes)
    ind = e.bill_report(baseline="individual")
    unc = e.bill_report(baseline="uncontrolled", baseline_fill="full")
    assert ind.keep.tobytes() == unc.keep.tobytes() and ind.keep[S:].sum() > 1000
    c_ind, c_unc, keep = ind.bill[S:], unc.bill[S:], ind.keep[S:].astype(bool)
    dev = 100 * (c_unc - c_ind) / c_ind
    empty = np.stack([(h["ev"] != 0) & ((h["nmin"] > h["nmax"]) | (h["nmax"] < 0)) for h in homes])
    assert (empty & ~keep).sum() == 0 and (keep & ~empty).sum() > 500
    print("kept", keep.sum(), "with empty rows", empty.sum(), "dev min", dev[keep & ~empty].min(), "max", dev[keep].max())
    assert (dev[keep & ~empty] >= -1e-9).all() and (dev[keep & ~empty] > 0.1).any()
    assert c_unc[empty].tobytes() == br.bills(load, tariff)[empty].tobytes()


def test_rule_calls_leave_the_state_alone(gpu_lib):
    w = _workload()
    homes = _mixed_scenarios(w, S)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for e in (a, b):
        e.run_steps(3)
    g = b.rule_schedule()
    b.study_report(groups=[0, 0, 1, 1, -1], profile=g)
    b.bill_report(baseline="uncontrolled", groups=[0, 0, 1, 1, -1])
    a.step()
    b.step()
    b.rule_schedule("trickle", "full")
    b.bill_report(baseline="last_minute", baseline_fill="full")
    a.step()
    b.step()
    assert a.iteration == b.iteration == 5
    for s in range(S):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
        assert a.multipliers(s).tobytes() == b.multipliers(s).tobytes(), s
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()


def test_study_with_a_rule_method_on_both_paths(gpu_lib, golden):
    """REVS.study on the 121144 feeder, 2 seeds x {distributed, individual, uncontrolled}: the rule rows, their network
    records and their bills are the same on the host path and on the device_report path, and count their unserved."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    res = [int(h) for h in z["res_id"]]
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    grid = dict(adoptions=(50,), ratings=(4800,), seeds=(1, 2), methods=("distributed", "individual", "uncontrolled"),
                max_iterations=2, bills=True, arrays=True, v0=1.03)
    lab0, rep0 = fx.study(tariff, all_homes, dist, com, **grid)
    lab1, rep1 = fx.study(tariff, all_homes, dist, com, ensemble=True, device_report=True, **grid)
    strip = lambda labs: [{k: v for k, v in lab.items() if k != "certificate"} for lab in labs]
    assert strip(lab0) == strip(lab1)
    assert [lab["method"] for lab in lab0] == ["distributed", "individual", "uncontrolled"] * 2
    rule = [2, 5]
    for lab in lab0:
        assert ("unserved" in lab) == (lab["method"] == "uncontrolled")
    assert [lab0[s]["unserved"] for s in rule] == [0, 0]                      # 4.8 kW over 11 .. 22 serves every EV
    for rep in (rep0, rep1):
        assert rep.groups.tolist() == [0, 1, 2] * 2 and rep.n_groups == 3
        assert rep.bills.base.tolist() == [1, 1, 1, 4, 4, 4]
        assert rep.bills.keep.sum(1).tolist() == [int(0.5 * len(com))] * 6
    assert rep0.node_p.shape == (6, len(res), 24)
    assert rep0.node_p[rule].tobytes() == rep1.node_p[rule].tobytes() and (rep0.node_p[2] != rep0.node_p[1]).any()
    for k in ("summary_volt", "summary_loading", "band_counts", "volt", "flow"):
        assert getattr(rep0, k)[rule].tobytes() == getattr(rep1, k)[rule].tobytes(), k
    for k in ("bill", "dev", "summary_bill", "summary_dev"):
        assert getattr(rep0.bills, k)[rule].tobytes() == getattr(rep1.bills, k)[rule].tobytes(), k
    # against the individual optimum uncontrolled charging costs every EV residence at least as much
    keep = rep0.bills.keep[rule].astype(bool)
    assert (rep0.bills.dev[rule][keep] >= -1e-9).all() and (rep0.bills.dev[rule][keep] > 0).any()
    # ... and with uncontrolled charging as the baseline the individual rows show the saving
    lab2, rep2 = fx.study(tariff, all_homes, dist, com, bill_base="uncontrolled", **grid)
    assert rep2.bills.base.tolist() == [2, 2, 2, 5, 5, 5]
    assert (rep2.bills.dev[[1, 4]][rep2.bills.keep[[1, 4]].astype(bool)] <= 1e-9).all()
