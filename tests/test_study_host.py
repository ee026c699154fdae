"""REVS.study and study.study_report on the host: the grid, the labels, the EV draw, the grouping and the bar-chart
helpers, with the device call replaced by the numpy yard-stick (tests/study_ref.py) the way test_network_host
replaces report_for_tree, and the optimisers by host stand-ins.  The kernels are the GPU tests' job.  No GPU."""
import numpy as np
import pytest

import network_ref as nr
import study_ref as sr
from test_network_host import LINES, golden_graph

TAGS = ("dis_a90_r4800", "ind_a90_r4800", "ind_a70_r4800", "ind_a90_r3600", "cen_a90_r4800")


@pytest.fixture()
def host_revs(golden, monkeypatch):
    """-> (fx, tariff, all_homes, dist, community, line table, calls): a REVS whose optimisers run on the host (the
    individual one is the oracle's; the distributed stand-in spreads every EV's energy evenly over its window) and
    record the homes they were given."""
    from oracle import revs_oracle as ro
    from revs_admm_amd import study
    from revs_admm_amd.lpsolver import homes_to_arrays
    from revs_admm_amd.revs_fixture import REVS
    z, fd = golden
    monkeypatch.setattr(study, "native_study", sr.host_study)
    fx = REVS(device="cpu")
    calls = []

    def individual(tariff, homes, save=False, **kw):
        keys = list(homes)
        load, rec = homes_to_arrays(homes, keys)
        p, s, g = ro.solve_residence(np.asarray(tariff, float), ro.homes_from_records(load, rec))
        calls.append(("individual", homes))
        return {h: g[i] for i, h in enumerate(keys)}, None, None

    def distributed(tariff, homes, dist, save=False, **kw):
        calls.append(("distributed", homes, kw))
        out = {}
        for h, d in homes.items():
            g = np.array(d["LOAD"], float)
            if d["EV"]:
                e = d["EV"]
                g[e["start"]:e["end"] + 1] += 0.7 * e["capacity"] / (e["end"] + 1 - e["start"])
            out[h] = g.tolist()
        return out, None, None

    monkeypatch.setattr(fx, "get_individual_optimal", individual)
    monkeypatch.setattr(fx, "get_distributed_optimal", distributed)
    ln = np.load(LINES)
    table = {s.decode(): float(r) for s, r in zip(ln["type_name"], ln["type_rating"])}
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], z["LOAD"])}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    return fx, z["tariff_shift6"], all_homes, golden_graph(golden), com, table, calls


def test_grid_order_labels_and_ev_draw(golden, host_revs):
    fx, tariff, all_homes, dist, com, table, calls = host_revs
    z = golden[0]
    labels, rep = fx.study(tariff, all_homes, dist, com, adoptions=(90, 30), ratings=(4800, 3600), seeds=(1234, 56),
                           line_rating=table, max_iterations=3)
    want = [dict(method=m, adoption=a, rating=r, seed=s) for a in (90, 30) for r in (4800, 3600) for s in (1234, 56)
            for m in ("distributed", "individual")]
    assert labels == want and [c[0] for c in calls] == [w["method"] for w in want]
    assert calls[0][2]["max_iterations"] == 3 and "feeder" in calls[0][2]
    assert all(c[2]["feeder"] is calls[0][2]["feeder"] for c in calls if c[0] == "distributed")      # formed once
    # (90, 1234): the reference's own draw, as stored with its result
    ev = [h for h, d in calls[0][1].items() if d["EV"]]
    assert sorted(ev) == sorted(int(h) for h in z["dis_a90_r4800_ev_homes"]) and len(ev) == int(0.9 * len(com)) == 267
    assert calls[0][1][ev[0]]["EV"] == dict(rating=4.8, capacity=20.0, initial=0.2, start=11, end=23)
    assert calls[4][1][ev[0]]["EV"]["rating"] == 3.6            # (rating 3600 W, the same seed: the same draw)
    # both methods of one (adoption, rating, seed) get the same homes; another seed draws others
    assert calls[0][1] is calls[1][1]
    ev56 = [h for h, d in calls[2][1].items() if d["EV"]]
    assert len(ev56) == 267 and sorted(ev56) != sorted(ev)
    assert len([h for h, d in calls[8][1].items() if d["EV"]]) == int(0.3 * len(com))
    assert rep.groups.tolist() == [0, 1] * 8 and rep.n_groups == 2
    assert rep.summary_volt.shape == (16, 24) and rep.pooled_volt.shape == (2, 24) and rep.band_counts.shape == (16, 24, 3)
    assert (rep.summary_volt["count"] == len(com)).all() and (rep.pooled_volt["count"] == 8 * len(com)).all()
    assert (rep.summary_loading["count"] == 1691).all() and (rep.pooled_loading["count"] == 8 * 1691).all()
    assert rep.volt is None and rep.bands == (0.92, 0.95, 0.98)


@pytest.mark.parametrize("group_by, n_groups", [("method", 2), ("adoption", 2), ("rating", 1), ("seed", 3),
                                                (("method", "adoption"), 4), (("adoption", "method"), 4)])
def test_grouping(host_revs, group_by, n_groups):
    fx, tariff, all_homes, dist, com, table, calls = host_revs
    labels, rep = fx.study(tariff, all_homes, dist, com, adoptions=(30, 90), ratings=(4800,), seeds=(1, 2, 3),
                           group_by=group_by, bands=(0.99, 0.97))
    keys = (group_by,) if isinstance(group_by, str) else group_by
    seen = []
    for lab, g in zip(labels, rep.groups):
        c = tuple(lab[k] for k in keys)
        if c not in seen:
            seen.append(c)
        assert g == seen.index(c)                             # (groups in order of first appearance)
    assert rep.n_groups == len(seen) == n_groups
    for g in range(n_groups):
        assert (rep.pooled_volt[g]["count"] == len(com) * (rep.groups == g).sum()).all()
    # unrated graph, no table: the loading records are empty
    assert (rep.summary_loading["count"] == 0).all() and (rep.pooled_loading["worst_scenario"] == -1).all()
    # the bar chart's numbers
    mean, (lo, hi) = rep.band_mean(), rep.band_range()
    assert mean.shape == lo.shape == hi.shape == (n_groups, 24, 2)
    for g in range(n_groups):
        c = rep.band_counts[rep.groups == g]
        assert np.array_equal(mean[g], c.mean(0)) and np.array_equal(lo[g], c.min(0)) and np.array_equal(hi[g], c.max(0))
    assert (lo <= mean).all() and (mean <= hi).all() and rep.band_counts.max() > 0
    assert (rep.band_counts[..., 0] >= rep.band_counts[..., 1]).all()       # cumulative, thresholds in any order


def test_unknown_group_key_or_method(host_revs):
    fx, tariff, all_homes, dist, com, table, calls = host_revs
    with pytest.raises(ValueError, match="'hour'"):
        fx.study(tariff, all_homes, dist, com, (30,), (4800,), (1,), group_by="hour")
    with pytest.raises(ValueError, match="'centralized'"):
        fx.study(tariff, all_homes, dist, com, (30,), (4800,), (1,), methods=("centralized",))
    assert calls == []


def test_band_counts_of_the_stored_results(golden, monkeypatch):
    """The five stored results as one study through study_report (yard-stick in place of the device): the counts at
    <= 0.92 / 0.95 / 0.98 over community 2 equal those of the dense float64 voltages -- recomputed here -- and tell the
    reference's story: the individual optimum at 90 % drives residences below 0.92, the distributed one none below
    0.95, the centralized one none below 0.98.  Pooling matters: the pooled quartile of the three individual results is
    none of the three per-result quartiles."""
    from revs_admm_amd import study
    from test_network_host import golden_tree
    monkeypatch.setattr(study, "native_study", sr.host_study)
    z, fd = golden
    g, res, nonsub, (par, er, cons), child, sign = golden_tree(golden)
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    nodes = [nonsub.index(h) for h in com]
    assert len(com) == 297
    rep = study.study_report(par, er, cons, np.stack([z[t + "_P_res"] for t in TAGS]), groups=[-1, 0, 0, 0, -1],
                             nodes=nodes, arrays=True, device="cpu")
    A_inv, R = nr.dense(fd.n_nodes, fd.edge_u, fd.edge_v, fd.edge_r, fd.nonsub())
    rows = [nonsub.index(h) for h in res]
    dense = []
    for t in TAGS:
        P = np.zeros((len(nonsub), 24))
        P[rows] = z[t + "_P_res"]
        dense.append(nr.volt(R, P, 1.0))
    dense = np.stack(dense)
    assert min(np.abs(dense[:, nodes] - b).min() for b in rep.bands) > 1e-9       # (no count hangs on rounding)
    assert np.array_equal(rep.band_counts, sr.band_counts(dense, nodes, (0.92, 0.95, 0.98)))
    c = {t: rep.band_counts[i, 20:23] for i, t in enumerate(TAGS)}
    print({t: v.tolist() for t, v in c.items()})
    assert (np.diff(rep.band_counts, axis=2) >= 0).all()
    assert c["ind_a90_r4800"][0, 0] > 0 and c["ind_a90_r4800"][0, 0] < c["ind_a90_r4800"][0, 1] < c["ind_a90_r4800"][0, 2]
    assert (c["dis_a90_r4800"][:, :2] == 0).all() and (c["dis_a90_r4800"][:, 2] > 0).all()
    assert (c["dis_a90_r4800"][:, 2] < c["ind_a90_r4800"][:, 2]).all()
    assert (c["cen_a90_r4800"] == 0).all()
    assert c["ind_a70_r4800"][0, 0] == 0 < c["ind_a70_r4800"][0, 1] < c["ind_a90_r4800"][0, 1]
    q1 = rep.pooled_volt["q1"][0, 20]
    each = rep.summary_volt["q1"][1:4, 20]
    assert each.min() < q1 < each.max() and (each != q1).all()
    assert rep.pooled_volt["count"][0, 20] == 3 * 297
