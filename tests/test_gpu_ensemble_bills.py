"""AdmmEnsemble.bill_report and REVS.study(bills=True) on the GPU (revs_admm_amd/ensemble_bills.py, DESIGN.md section
3.10): the report from the state on the device is, bit for bit, bills.bill_report fed the schedules the ensemble
returns and the individual optimum of the same records; the run's state is left alone; the study's BillReport is the
same on the host path and on the device_report path."""
import numpy as np
import pytest

import bills_ref as br
from test_gpu_ensemble import _ensemble, _mixed_scenarios, _workload
from test_gpu_ensemble_report import _mixed_ensemble

pytestmark = pytest.mark.gpu


def test_ensemble_bill_report(gpu_lib):
    from revs_admm_amd import bills
    from revs_admm_amd.engine import residence_solve
    w, load, e = _mixed_ensemble(3)
    homes = _mixed_scenarios(w, 5)
    S, n, T = 5, 600, 24
    groups = [0, 0, 1, 1, -1]
    rep = e.bill_report(baseline="individual", groups=groups)
    P = e.result()[0]
    assert P.shape == (S, n, T) and P.dtype == np.float32
    # the individual optimum of the same records (lpsolver.solve_residences' batched core), float32 like the schedules
    ind = np.stack([residence_solve(w.cost, homes[s], load[s])[2] for s in range(S)])
    assert ind.dtype == np.float32
    ev = np.stack([homes[s]["ev"] != 0 for s in range(S)])
    tariff = np.asarray(w.cost, np.float32).astype(np.float64)
    ref = bills.bill_report(np.concatenate([P, ind]), tariff, base=list(range(S, 2 * S)) + [-1] * S,
                            groups=groups + [-1] * S, keep=np.concatenate([ev, ev]))
    br.same_report(rep, ref)
    assert rep.bill.shape == (2 * S, n) and rep.n_groups == 2 and rep.base.tolist() == [5, 6, 7, 8, 9] + [-1] * 5
    # ... which is the numpy restatement's
    want = br.bills(np.concatenate([P, ind]), tariff)
    assert rep.bill.tobytes() == want.tobytes() and rep.dev.tobytes() == br.deviations(want, rep.base).tobytes()
    br.check_report(rep, rep.bill, rep.dev, rep.keep)
    # ev_only keeps exactly every scenario's EV owners; the scenarios differ in them
    assert rep.keep.tobytes() == np.concatenate([ev, ev]).tobytes() and (ev[0] != ev[1]).any()
    assert rep.summary_bill["count"].tolist() == (ev.sum(1).tolist()) * 2
    # worst_index in the caller's order
    for s in range(S):
        d = np.where(ev[s] & np.isfinite(rep.dev[s]), rep.dev[s], -np.inf)
        assert rep.summary_dev["worst_index"][s] == int(np.argmax(d)) and rep.summary_dev["worst_scenario"][s] == s
    # every residence, records only, an explicit baseline, none at all
    every = e.bill_report(groups=groups, ev_only=False, arrays=False)
    assert every.bill is None and every.keep is None and every.summary_bill["count"].tolist() == [n] * (2 * S)
    given = e.bill_report(baseline=ind.astype(np.float64), groups=groups)
    br.same_report(given, rep)
    none = e.bill_report(baseline=None, groups=groups)
    assert none.bill.tobytes() == rep.bill[:S].tobytes() and np.isnan(none.dev).all()
    assert none.summary_bill.tobytes() == rep.summary_bill[:S].tobytes()
    assert none.pooled_bill.tobytes() == rep.pooled_bill.tobytes() and (none.summary_dev["count"] == 0).all()
    with pytest.raises(ValueError, match="baseline must be"):
        e.bill_report(baseline="centralized")
    with pytest.raises(ValueError, match="caller's residence order"):
        e.bill_report(baseline=np.zeros((S, n, T + 1)))
    with pytest.raises(ValueError, match="groups must be 5 integers"):
        e.bill_report(groups=[0, 0])


def test_bill_report_leaves_the_state_alone(gpu_lib):
    w = _workload()
    homes = _mixed_scenarios(w, 5)
    a, b = (_ensemble(w, homes, "relaxed_exact") for _ in range(2))
    for e in (a, b):
        e.run_steps(3)
    b.bill_report(groups=[0, 0, 1, 1, -1])
    a.step()
    b.step()
    assert a.iteration == b.iteration == 4
    for s in range(5):
        for x, y in zip(a.get_state(s), b.get_state(s)):
            assert x.tobytes() == y.tobytes(), s
        assert a.multipliers(s).tobytes() == b.multipliers(s).tobytes(), s


def test_study_bills_on_both_paths(gpu_lib, golden):
    """REVS.study(bills=True) on the 121144 feeder, 2 seeds x {distributed, individual}: base pairs every distributed
    row with its individual sibling, keep is the scenario's EV homes, and the BillReport is bills.bill_report of the
    report's own rows on the host path and on the device_report path alike."""
    from helpers import f32
    from test_network_host import golden_graph
    from revs_admm_amd import bills
    from revs_admm_amd.revs_fixture import REVS
    z = golden[0]
    dist = golden_graph(golden)
    res = [int(h) for h in z["res_id"]]
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], f32(z["LOAD"]))}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    tariff = f32(z["tariff_shift6"])
    fx = REVS()
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), group_by="method", max_iterations=3, v0=1.03,
                arrays=True, mode="relaxed", bills=True)
    lab0, rep0 = fx.study(tariff, all_homes, dist, com, ensemble=True, **grid)
    lab1, rep1 = fx.study(tariff, all_homes, dist, com, ensemble=True, device_report=True, **grid)
    assert lab0 == lab1 and [l["method"] for l in lab0] == ["distributed", "individual"] * 2
    for rep in (rep0, rep1):
        b = rep.bills
        assert b.base.tolist() == [1, 1, 3, 3] and b.groups.tolist() == [0, 1, 0, 1] and b.n_groups == 2
        assert b.keep.shape == (4, len(res)) and b.keep.sum(1).tolist() == [int(90 * 1e-2 * len(com))] * 4
        assert (b.keep[0] == b.keep[1]).all() and (b.keep[0] != b.keep[2]).any()
        ref = bills.bill_report(rep.node_p, tariff, base=b.base, groups=b.groups, keep=b.keep)
        br.same_report(b, ref)
        br.check_report(b, b.bill, b.dev, b.keep)
        assert (b.dev[[1, 3]] == 0.0).all() and (b.summary_dev["count"] == 4 * [int(90 * 1e-2 * len(com))]).all()
    same = rep0.node_p.tobytes() == rep1.node_p.tobytes()
    print("the two paths' rows are", "identical" if same else "not identical")
    if same:
        br.same_report(rep0.bills, rep1.bills)
