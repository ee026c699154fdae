"""AdmmEnsemble.node_sums / study_report / network_reports on the host: the driver -- argument checks before any launch,
the caller's residence order into the engine's, the slice of a larger study buffer, the feeder's tree handed on -- over
the numpy stand-in of the kernels (tests/fake_kernels.py) with revs_net_node_sums_many restated here and
study.native_study_device replaced by tests/study_ref.py.  The kernel itself is tests/test_gpu_node_sums_many.py's
job, the report's bits tests/test_gpu_ensemble_report.py's."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

TREE_MESSAGE = "network_report needs the feeder as a tree"


def _fake():
    from fake_kernels import FakeKernels, view

    class FakeReport(FakeKernels):
        """+ revs_net_node_sums_many: load / p float[n][S][T], node_g double[S][m][T], one accumulator per output."""
        calls = []

        def revs_net_node_sums_many(self, S, m, T, node_ptr, load, p, node_g, stream):
            ptr = view(node_ptr, (m + 1,), np.int64)
            n = int(ptr[-1])
            pv = view(p, (n, S, T), np.float32)
            lv = view(load, (n, S, T), np.float32) if load else None
            type(self).calls.append(dict(S=S, m=m, T=T, p=pv.copy(), load=None if lv is None else lv.copy()))
            out = view(node_g, (S, m, T), np.float64)
            for node in range(m):
                acc = np.zeros((S, T))
                for i in range(ptr[node], ptr[node + 1]):
                    acc = acc + (pv[i].astype(np.float64) if lv is None
                                 else lv[i].astype(np.float64) + pv[i].astype(np.float64))
                out[:, node, :] = acc
            return 0
    FakeReport.calls = []
    return FakeReport


def _ensemble(S=3, feeder=True, n=90, T=24, nodes=12):
    from helpers import f32
    from test_ensemble_certificate_host import _scenarios
    from revs_admm_amd.ensemble import AdmmEnsemble
    from revs_admm_amd.synthetic import make_workload
    Fake = _fake()
    w = make_workload(n, T, n_nodes=nodes, seed=11, binary_feasible=False, stress=1.0)
    w.load, w.cost = f32(w.load), f32(w.cost)
    shuffle = np.random.default_rng(7).permutation(n)        # (make_workload lists the residences node by node)
    w.node_of, w.load = w.node_of[shuffle], w.load[shuffle]
    load = np.stack([w.load] * S)
    load[1] = f32(1.25 * w.load)
    e = AdmmEnsemble(w.cost, _scenarios(n, T, S), load, w.node_of, w.Rn, kappa=w.kappa, vset=w.vset, vlow=w.vlow,
                     vhigh=w.vhigh, mode="relaxed_exact", device="cpu", feeder=w.feeder if feeder else None,
                     _kernels=Fake())
    rng = np.random.default_rng(S)
    P = f32(load + rng.uniform(0.0, 2.0, load.shape) * (rng.random(load.shape) < 0.2))
    for s in range(S):
        e.set_state(s, P[s], P[s], np.zeros((n, T)))
    return w, load.astype(np.float32), P.astype(np.float32), e, Fake      # (f32 gives float values held in float64)


def _sums(w, prof64):
    """(S, n, T) float64 in the caller's order -> (S, M, T): within a node the engine keeps ascending index."""
    out = np.zeros((prof64.shape[0], w.M, prof64.shape[2]))
    for i in range(prof64.shape[1]):
        out[:, w.node_of[i], :] = out[:, w.node_of[i], :] + prof64[:, i, :]
    return out


def _host_study(w, seen):
    """study.native_study_device's stand-in: tests/study_ref.host_study on the node sums it is handed."""
    import study_ref as sr

    def native_study_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, groups, n_groups, bands, rating, nodes,
                            vset, vmin, vmax, arrays):
        par, er, cons = w.feeder
        seen.append(dict(tree=tree, tree_host=tree_host, n_nodes=n_nodes, groups=np.asarray(groups).tolist(),
                         n_groups=n_groups, bands=tuple(bands), vset=vset, vmin=vmin, vmax=vmax, arrays=arrays))
        assert n_nodes == len(par)
        return sr.host_study(par, er, cons, node_g.numpy().copy(), groups, n_groups, bands, rating, nodes, vset, vmin,
                             vmax, arrays)
    return native_study_device


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    from revs_admm_amd import study
    w, load, P, e, Fake = _ensemble()
    seen = []
    monkeypatch.setattr(study, "native_study_device", _host_study(w, seen))
    S, n, T = 3, 90, 24
    with pytest.raises(ValueError, match="groups must be 3 integers"):
        e.study_report(groups=[0, 1])
    with pytest.raises(ValueError, match="groups must be 3 integers"):
        e.study_report(groups=[0, 1, 0, 1])
    with pytest.raises(ValueError, match="at most 8 finite bands"):
        e.study_report(bands=tuple(0.9 + 0.01 * b for b in range(9)))
    with pytest.raises(ValueError, match="profile"):
        e.study_report(profile=np.zeros((n, S, T), np.float32))          # (the engine's layout as a host array: refused)
    with pytest.raises(ValueError, match="profile"):
        e.node_sums(profile=np.zeros((S, n, T + 1)))
    import torch
    with pytest.raises(ValueError, match="profile"):
        e.node_sums(profile=torch.zeros(n, S, T, dtype=torch.float64))
    with pytest.raises(ValueError, match="profile"):
        e.node_sums(profile=torch.zeros(S, n, T))
    with pytest.raises(ValueError, match="out must be"):
        e.node_sums(out=torch.zeros(S, w.M + 1, T, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        e.node_sums(out=torch.zeros(S, w.M, T))
    with pytest.raises(ValueError, match="out must be"):
        e.node_sums(out=torch.zeros(w.M, S, T, dtype=torch.float64).transpose(0, 1))
    assert Fake.calls == [] and seen == []


def test_without_the_tree_the_reports_say_what_network_report_says():
    from revs_admm_amd.engine import AdmmEngine
    w, load, P, e, Fake = _ensemble(feeder=False)
    assert e._tree is None
    with pytest.raises(ValueError, match=TREE_MESSAGE) as a:
        e.study_report()
    with pytest.raises(ValueError, match=TREE_MESSAGE):
        e.network_reports()
    assert Fake.calls == []
    plain = type("Plain", (), {"_tree": None})()
    with pytest.raises(ValueError, match=TREE_MESSAGE) as b:
        AdmmEngine.network_report(plain)
    assert str(a.value) == str(b.value)
    # the node sums need no tree
    g = e.node_sums().numpy()
    assert g.tobytes() == _sums(w, P.astype(np.float64)).tobytes()


def test_profiles_reach_the_kernel_in_the_engines_order():
    import torch
    w, load, P, e, Fake = _ensemble()
    S, n, T = 3, 90, 24
    assert not np.array_equal(e.perm, np.arange(n))                      # (the permutation is not the identity)
    # the default: P_sch alone, no load
    g = e.node_sums()
    assert isinstance(g, torch.Tensor) and g.dtype == torch.float64 and tuple(g.shape) == (S, w.M, T)
    call = Fake.calls[-1]
    assert (call["S"], call["m"], call["T"]) == (S, w.M, T) and call["load"] is None
    assert call["p"].tobytes() == np.ascontiguousarray(P.transpose(1, 0, 2)[e.perm]).tobytes()
    assert g.numpy().tobytes() == _sums(w, P.astype(np.float64)).tobytes()
    # a host profile in the caller's order, the engine's load added
    ev = np.random.default_rng(1).uniform(0.0, 7.2, (S, n, T)).astype(np.float32)
    g = e.node_sums(profile=ev, add_load=True)
    call = Fake.calls[-1]
    for k in range(n):
        assert call["p"][k].tobytes() == ev[:, e.perm[k], :].tobytes(), k
        assert call["load"][k].tobytes() == load[:, e.perm[k], :].tobytes(), k
    assert g.numpy().tobytes() == _sums(w, load.astype(np.float64) + ev.astype(np.float64)).tobytes()
    # a tensor in the engine's layout goes through as it is
    t = torch.from_numpy(np.ascontiguousarray(ev.transpose(1, 0, 2)[e.perm]))
    assert e.node_sums(profile=t, add_load=True).numpy().tobytes() == g.numpy().tobytes()
    assert len(Fake.calls) == 3


def test_out_fills_its_slice_and_nothing_else():
    import torch
    w, load, P, e, Fake = _ensemble()
    S, T = 3, 24
    buf = torch.full((S + 4, w.M, T), float("nan"), dtype=torch.float64)
    got = e.node_sums(out=buf[2:2 + S])
    assert got.data_ptr() == buf[2].data_ptr()
    b = buf.numpy()
    assert np.isnan(b[:2]).all() and np.isnan(b[2 + S:]).all()
    assert b[2:2 + S].tobytes() == _sums(w, P.astype(np.float64)).tobytes()


def test_the_report_on_the_host_stand_in(monkeypatch):
    from revs_admm_amd import study
    from network_worker import line_ratings
    w, load, P, e, Fake = _ensemble()
    seen = []
    monkeypatch.setattr(study, "native_study_device", _host_study(w, seen))
    rating, nodes = line_ratings(w)
    state = [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)]
    rep = e.study_report(groups=[1, 0, 1], rating=rating, nodes=nodes, arrays=True)
    assert len(Fake.calls) == 1 and len(seen) == 1
    k = seen[0]
    assert k["tree"] is e._tree and k["tree_host"] is e._tree_host and k["groups"] == [1, 0, 1] and k["n_groups"] == 2
    assert k["bands"] == (0.92, 0.95, 0.98) and (k["vset"], k["vmin"], k["vmax"]) == (e.vset, e.vlow, e.vhigh)
    sums = _sums(w, P.astype(np.float64))
    assert rep.node_p.tobytes() == sums.tobytes() and rep.n_groups == 2 and rep.volt.shape == (3, len(w.feeder[0]), 24)
    # the limits can be overridden, as study_report's
    e.study_report(vset=1.0, vmin=0.9, vmax=1.1, bands=(0.95,))
    assert (seen[1]["vset"], seen[1]["vmin"], seen[1]["vmax"]) == (1.0, 0.9, 1.1) and seen[1]["bands"] == (0.95,)
    assert seen[1]["n_groups"] == 0 and not seen[1]["arrays"]
    # the per-scenario reports: one launch, no pools, no bands
    reports = e.network_reports(rating=rating, nodes=nodes)
    assert len(reports) == 3 and len(Fake.calls) == 3 and len(seen) == 3
    assert seen[2]["n_groups"] == 0 and seen[2]["bands"] == () and seen[2]["arrays"]
    for s, r in enumerate(reports):
        assert r.node_sums.tobytes() == sums[s].tobytes()
        assert r.volt.tobytes() == rep.volt[s].tobytes() and r.flow.tobytes() == rep.flow[s].tobytes()
        assert r.summary_volt.tobytes() == rep.summary_volt[s].tobytes()
        assert r.summary_loading.tobytes() == rep.summary_loading[s].tobytes()
        assert (r.vset, r.vmin, r.vmax) == (e.vset, e.vlow, e.vhigh)
    none = e.network_reports(arrays=False)
    assert none[0].volt is None and none[0].flow is None and none[0].loading is None
    for a, b in zip(state, (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_the_singular_methods_still_raise():
    from revs_admm_amd.ensemble import AdmmEnsemble
    for name in ("lower_bound", "certificate", "network_report", "voltage"):
        with pytest.raises(NotImplementedError, match=r"lower_bounds\(\) / certificates\(\)") as err:
            getattr(AdmmEnsemble, name)(None)
        assert "study_report()" in str(err.value) and "network_reports()" in str(err.value)


def test_study_device_report_needs_the_ensemble(golden):
    """REVS.study(device_report=True) without ensemble=True is refused before anything is solved."""
    from test_network_host import golden_graph
    from revs_admm_amd.revs_fixture import REVS
    z, _ = golden
    dist = golden_graph(golden)
    all_homes = {int(h): row.tolist() for h, row in zip(z["res_id"], z["LOAD"])}
    com = [int(h) for h in z["com_flat"][z["com_offsets"][1]:z["com_offsets"][2]]]
    with pytest.raises(ValueError, match="device_report=True.*ensemble=True"):
        REVS(device="cpu").study(z["tariff_shift6"].tolist(), all_homes, dist, com, adoptions=(30,), ratings=(4800,),
                                 seeds=(1234,), device_report=True)
