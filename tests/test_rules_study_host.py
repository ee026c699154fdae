"""REVS.study with rule methods on the host, in the way of tests/test_study_host.py: the labels, the groups, the number
of unserved residences and the baseline row of the bill report, with the device calls replaced by numpy yard-sticks
(study_ref.host_study, rules_ref.rule_schedule).  The kernels are the GPU tests' job.  No GPU."""
import numpy as np
import pytest

import rules_ref as rr
from test_study_host import host_revs  # noqa: F401  (the fixture)


@pytest.fixture()
def rule_revs(host_revs, monkeypatch):  # noqa: F811
    """host_revs with lpsolver.solve_uncontrolled as REVS.study calls it replaced by the restatement, and the bill
    report by a recorder of its arguments."""
    from revs_admm_amd import bills, revs_fixture
    from revs_admm_amd.lpsolver import homes_to_arrays
    fx, tariff, all_homes, dist, com, table, calls = host_revs
    seen = dict(rule=[], bills=[])

    def uncontrolled(homes, T=None, policy="uncontrolled", fill="target", charger="binary", device=None,
                     return_status=False):
        keys = list(homes)
        load, rec = homes_to_arrays(homes, keys)
        integral = 1 if charger == "binary" else 0
        p, s, g, status = rr.rule_schedule(rec, load, rr.POLICY[policy], rr.FILL[fill], integral)
        seen["rule"].append(dict(policy=policy, fill=fill, charger=charger, T=T, homes=homes))
        calls.append((policy, homes))
        sol = {h: (p[i], s[i], g[i]) for i, h in enumerate(keys)}
        return (sol, {h: int(status[i]) for i, h in enumerate(keys)}) if return_status else sol

    def bill_report(g, tariff, **kw):
        seen["bills"].append(dict(g=g, **kw))
        return "bills"

    monkeypatch.setattr(revs_fixture, "solve_uncontrolled", uncontrolled)
    monkeypatch.setattr(bills, "bill_report", bill_report)
    return fx, tariff, all_homes, dist, com, seen, calls


def test_rule_methods_are_labelled_grouped_and_pooled(rule_revs):
    fx, tariff, all_homes, dist, com, seen, calls = rule_revs
    methods = ("distributed", "individual", "uncontrolled", "last_minute")
    labels, rep = fx.study(tariff, all_homes, dist, com, adoptions=(50,), ratings=(4800,), seeds=(1, 2), methods=methods,
                           bills=True, rule_fill="full")
    assert [lab["method"] for lab in labels] == list(methods) * 2
    assert [c[0] for c in calls] == list(methods) * 2
    assert calls[2][1] is calls[0][1] and calls[3][1] is calls[1][1]          # the same homes for every method of a case
    assert rep.groups.tolist() == [0, 1, 2, 3] * 2 and rep.n_groups == 4
    assert (rep.pooled_volt["count"] == 2 * len(com)).all() and rep.bills == "bills"
    for lab in labels:
        assert ("unserved" in lab) == (lab["method"] in ("uncontrolled", "last_minute"))
    # 4.8 kW into 20 kWh from 0.2 over slots 11 .. 22: every EV is served
    assert [lab["unserved"] for lab in labels if "unserved" in lab] == [0, 0, 0, 0]
    assert all(r["fill"] == "full" and r["charger"] == "binary" and r["T"] == 24 for r in seen["rule"])
    # the rule rows are the restatement's net load of those homes
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    from revs_admm_amd.lpsolver import homes_to_arrays
    load, rec = homes_to_arrays(seen["rule"][0]["homes"], res)
    g = rr.rule_schedule(rec, load, rr.ASAP, rr.FULL, 1)[2]
    b, = seen["bills"]
    assert np.array_equal(b["g"][2], g.astype(np.float64)) and (b["g"][2] != b["g"][3]).any()
    # the baseline of every row: the individual row of its (adoption, rating, seed)
    assert list(b["base"]) == [1, 1, 1, 1, 5, 5, 5, 5] and list(b["groups"]) == [0, 1, 2, 3] * 2
    ev = np.isin(res, [h for h, d in seen["rule"][0]["homes"].items() if d["EV"]])
    assert np.array_equal(b["keep"][2], ev) and ev.sum() == int(0.5 * len(com))


def test_bill_base_picks_the_baseline_row(rule_revs):
    fx, tariff, all_homes, dist, com, seen, calls = rule_revs
    kw = dict(adoptions=(30, 50), ratings=(4800,), seeds=(7,), bills=True)
    fx.study(tariff, all_homes, dist, com, methods=("individual", "uncontrolled"), bill_base="uncontrolled", **kw)
    assert list(seen["bills"][-1]["base"]) == [1, 1, 3, 3]
    fx.study(tariff, all_homes, dist, com, methods=("individual", "trickle"), mode="relaxed", **kw)
    assert list(seen["bills"][-1]["base"]) == [0, 0, 2, 2] and seen["rule"][-1]["charger"] == "relaxed"
    fx.study(tariff, all_homes, dist, com, methods=("uncontrolled",), **kw)   # no individual row: no baseline
    assert list(seen["bills"][-1]["base"]) == [-1, -1]
    labels, _ = fx.study(tariff, all_homes, dist, com, methods=("uncontrolled",), adoptions=(50,), ratings=(1200,),
                         seeds=(3,), end_time=13)
    assert labels[0]["unserved"] == int(0.5 * len(com))         # 1.2 kW over two slots: nobody reaches 90 %


def test_unknown_names_still_raise(rule_revs):
    fx, tariff, all_homes, dist, com, seen, calls = rule_revs
    with pytest.raises(ValueError, match="'centralized'"):
        fx.study(tariff, all_homes, dist, com, (30,), (4800,), (1,), methods=("uncontrolled", "centralized"))
    with pytest.raises(ValueError, match="'asap'"):
        fx.study(tariff, all_homes, dist, com, (30,), (4800,), (1,), methods=("asap",))
    with pytest.raises(ValueError, match="'centralized'"):
        fx.study(tariff, all_homes, dist, com, (30,), (4800,), (1,), methods=("uncontrolled",), bill_base="centralized")
    assert calls == []
