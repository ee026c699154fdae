"""Statistics across scenarios on the host: the numpy yard-stick (tests/across_ref.py) against cells worked by hand, and
the Python layers -- study.study_report / study_report_device / across_report_device, AdmmEnsemble.study_report,
REVS.study -- with the library's entries replaced by the stand-ins (study.native_across by across_ref.host_across, the
report by tests/study_ref.py).  The kernels are tests/test_gpu_across.py's job.  No GPU."""
import numpy as np
import pytest

import across_ref as ar
from test_study_host import host_revs  # noqa: F401  (a fixture)

NAN, INF = float("nan"), float("inf")


def _rec(r):
    return ([float(r[k]) for k in ar.QS + ("mean",)],
            [int(r[k]) for k in ("count", "n_nan", "n_violations", "worst_scenario")], r["band_count"].tolist())


@pytest.mark.parametrize("v, scen, want", [
    # lo = 1.5, hi = 3.5, sense +1, bands (2.0, 4.0): values at or above
    ([3.0], [7], ([3.0, 3.0, 3.0, 3.0, 3.0, 3.0], [1, 0, 0, 7], [1, 0])),
    ([2.0, 1.0], [4, 9], ([1.0, 1.25, 1.5, 1.75, 2.0, 1.5], [2, 0, 1, 9], [1, 0])),
    ([4.0, 1.0, 3.0, 2.0], None, ([1.0, 1.75, 2.5, 3.25, 4.0, 2.5], [4, 0, 2, 0], [3, 1])),        # (a tie of excursions 0.5)
    ([5.0, 1.0, 4.0, 2.0, 3.0], None, ([1.0, 2.0, 3.0, 4.0, 5.0, 3.0], [5, 0, 3, 0], [4, 2])),
    ([2.0, 2.0, 2.0, 1.0], None, ([1.0, 1.75, 2.0, 2.0, 2.0, 1.75], [4, 0, 1, 3], [3, 0])),         # ties
    ([1.0, NAN, 3.0], [2, 5, 6], ([1.0, 1.5, 2.0, 2.5, 3.0, 2.0], [2, 1, 1, 2], [1, 0])),
    ([NAN, NAN], None, ([NAN] * 6, [0, 2, 0, -1], [0, 0])),
    ([], None, ([NAN] * 6, [0, 0, 0, -1], [0, 0])),
])
def test_yardstick_on_hand_worked_cells(v, scen, want):
    d, i, b = _rec(ar.cell(v, 1.5, 3.5, 1, (2.0, 4.0), scen))
    assert ar.same_numbers(d, want[0]) and i == want[1] and b[:2] == want[2] and b[2:] == [0] * 6


def test_yardstick_voltage_sense_daily_and_exposure():
    # two nodes, three slots; group 0 = scenarios 0 and 2, scenario 1 in no group
    v = np.array([[[1.00, 0.94, 0.96], [1.0, NAN, 1.0]],
                  [[0.50, 0.50, 0.50], [0.5, 0.5, 0.5]],
                  [[0.93, 0.99, 1.06], [1.0, 1.0, 0.9]]])
    slot, daily, expo = ar.across(v, None, [0, -1, 0], 1, 0.95, 1.05, -1, (0.95,))
    assert slot.shape == (1, 2, 3) and daily.shape == (1, 2) and expo.tolist() == [[3, 1]]
    assert slot["n_violations"][0].tolist() == [[1, 1, 1], [0, 0, 1]] and slot["n_nan"][0, 1].tolist() == [0, 1, 0]
    assert slot["worst_scenario"][0].tolist() == [[2, 0, 2], [0, 2, 2]]
    assert slot["band_count"][0, :, :, 0].tolist() == [[1, 1, 0], [0, 0, 1]]
    # the daily minima: node 0: 0.94 and 0.93; node 1: a NaN (scenario 0 has one) and 0.9
    assert np.allclose(_rec(daily[0, 0])[0][:5], [0.93, 0.9325, 0.935, 0.9375, 0.94], rtol=0, atol=1e-15)
    assert (daily["count"][0].tolist(), daily["n_nan"][0].tolist()) == ([2, 1], [0, 1])
    assert daily["band_count"][0, :, 0].tolist() == [2, 1] and daily["min"][0, 1] == 0.9
    # keep: node 1 left out -> the empty record, its NaN uncounted
    slot, daily, expo = ar.across(v, np.array([True, False]), [0, -1, 0], 1, 0.95, 1.05, -1, (0.95,))
    assert slot[0, 1].tobytes() == ar.empty((3,)).tobytes() and daily[0, 1].tobytes() == ar.empty(()).tobytes()
    assert expo.tolist() == [[3, 0]]
    # the vectorised cells are the cell-by-cell ones
    rng = np.random.default_rng(3)
    w = np.round(rng.normal(1.0, 0.05, (7, 4, 5)) * 1024) / 1024
    whole = ar.across_cells(w, None, [0, 1, 0, 1, 1, 0, -1], 2, 0.95, 1.05, -1, (0.92, 0.95, 0.98))
    for g, mem in enumerate(([0, 2, 5], [1, 3, 4])):
        for i in range(4):
            for t in range(5):
                assert whole[g, i, t].tobytes() == ar.cell(w[mem, i, t], 0.95, 1.05, -1, (0.92, 0.95, 0.98), mem).tobytes()


@pytest.fixture()
def seam(monkeypatch):
    from revs_admm_amd import study
    monkeypatch.setattr(study, "native_across", ar.host_across)
    ar.CALLS.clear()
    return ar.CALLS


def _forest(S=6, M=40, T=5, seed=2):
    from test_gpu_network import synthetic_forest
    rng = np.random.default_rng(seed)
    par, er, cons = synthetic_forest(M, seed=seed)
    p = rng.uniform(0.0, 1.5e-3, (S, M, T)) * rng.uniform(0.3, 1.0, (S, 1, 1))      # (volts of 0.8 .. 1)
    rating = np.where(rng.random(len(par)) < 0.8, rng.uniform(0.004, 0.04, len(par)), 0.0)
    nodes = np.sort(rng.choice(len(par), len(par) // 2, replace=False))
    return (par, er, cons), p, rating, nodes


def test_study_report_passes_across_through(seam, monkeypatch):
    from revs_admm_amd import study
    monkeypatch.setattr(study, "native_study", ar.host_study)
    feeder, p, rating, nodes = _forest()
    groups = [0, 1, 0, -1, 1, 0]
    rep = study.study_report(*feeder, p, groups=groups, rating=rating, nodes=nodes, bands=(0.9, 0.97), arrays=True,
                             device="cpu", across=True)
    assert isinstance(rep.across, study.AcrossReport) and len(seam) == 2
    n = len(feeder[0])
    volt_call, load_call = seam
    assert volt_call["shape"] == (6, n, 5) and (volt_call["lo"], volt_call["hi"], volt_call["sense"]) == (0.95, 1.05, -1)
    assert volt_call["bands"] == (0.9, 0.97) and volt_call["groups"] == groups and volt_call["n_groups"] == 2
    assert np.flatnonzero(volt_call["keep"]).tolist() == nodes.tolist()
    assert (load_call["lo"], load_call["hi"], load_call["sense"], load_call["bands"]) == (-INF, 1.0, 1, (0.8, 1.0))
    assert np.array_equal(load_call["keep"], rating > 0) and volt_call["slots"] and load_call["slots"]
    ar.check_report(rep.across, rep.volt, rep.loading, groups, nodes, rating, (0.9, 0.97), (0.8, 1.0), 0.95, 1.05)
    assert rep.across.slot_volt.shape == (2, n, 5) and rep.across.daily_loading.shape == (2, n)
    assert rep.across.exposure_volt.dtype == np.int32 and rep.across.group_sizes.tolist() == [3, 2]
    assert rep.across.slot_volt["count"].max() == 3 and rep.across.slot_volt["n_violations"].max() > 0      # (not trivial)
    # without arrays the report is the same and the arrays are not kept; without ratings there are no loading records
    lean = study.study_report(*feeder, p, groups=groups, rating=rating, nodes=nodes, bands=(0.9, 0.97), device="cpu",
                              across=True)
    assert lean.volt is None and ar.same_across(lean.across, rep.across)
    bare = study.study_report(*feeder, p, groups=groups, device="cpu", across=True)
    assert bare.across.slot_loading is None and bare.across.exposure_loading is None
    assert (bare.across.slot_volt["count"][0] == 3).all()


def test_across_needs_groups_and_the_default_calls_nothing(seam, monkeypatch):
    import study_ref as sr
    import torch
    from revs_admm_amd import study
    feeder, p, rating, nodes = _forest()
    called = []
    monkeypatch.setattr(study, "native_study", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError, match="across=True.*pass groups"):
        study.study_report(*feeder, p, across=True, device="cpu")
    with pytest.raises(ValueError, match="across=True.*pass groups"):
        study.study_report_device(torch.from_numpy(p), feeder=feeder, across=True)
    with pytest.raises(ValueError, match="no scenario is in a group"):
        study.study_report(*feeder, p, groups=[-1] * 6, across=True, device="cpu")
    with pytest.raises(ValueError, match="no scenario is in a group"):
        study.study_report_device(torch.from_numpy(p), feeder=feeder, groups=[-1] * 6, across=True)
    assert called == [] and seam == []
    # the default: the stand-ins with the signature before `across` are called as before, and nothing reaches the seam
    monkeypatch.setattr(study, "native_study", sr.host_study)
    rep = study.study_report(*feeder, p, groups=[0] * 6, rating=rating, nodes=nodes, device="cpu")
    assert rep.across is None and seam == []
    seen = []

    def old_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, groups, n_groups, bands, rating, nodes, vset, vmin,
                   vmax, arrays):
        seen.append(arrays)
        return sr.host_study(*feeder, node_g.numpy().copy(), groups, n_groups, bands, rating, nodes, vset, vmin, vmax, arrays)
    monkeypatch.setattr(study, "native_study_device", old_device)
    rep = study.study_report_device(torch.from_numpy(p), feeder=feeder, groups=[0] * 6, across=False)
    assert rep.across is None and seen == [False] and seam == []
    # StudyReport built positionally with the fields before `across` (tests/study_ref.host_study does) has none
    assert study.StudyReport(*[None] * 14).across is None


def test_study_report_device_passes_across_through(seam, monkeypatch):
    import torch
    from revs_admm_amd import study
    feeder, p, rating, nodes = _forest(S=4, T=3)
    seen = []
    monkeypatch.setattr(study, "native_study_device", ar.host_study_device(feeder, seen))
    rep = study.study_report_device(torch.from_numpy(p), feeder=feeder, groups=[1, 1, 0, 0], rating=rating, nodes=nodes,
                                    arrays=True, across=True)
    assert seen == [dict(arrays=True, across=True, n_groups=2)] and len(seam) == 2
    ar.check_report(rep.across, rep.volt, rep.loading, [1, 1, 0, 0], nodes, rating, (0.92, 0.95, 0.98), (0.8, 1.0), 0.95, 1.05)


def test_across_report_device_on_the_stand_in(seam):
    """across_report_device alone: slots=False, its own bands and limits, loading None."""
    import torch
    from revs_admm_amd import study
    rng = np.random.default_rng(8)
    volt = np.round(rng.normal(0.97, 0.03, (5, 6, 4)) * 1024) / 1024
    volt[1, 2, 3] = NAN
    load = np.round(rng.uniform(0.2, 1.3, (5, 6, 4)) * 1024) / 1024
    acr = study.across_report_device(torch.from_numpy(volt), torch.from_numpy(load), [0, 0, 1, 0, -1], nodes=[0, 2, 5],
                                     rated=[1.0, 0.0, 5.0, NAN, 2.0, 3.0], bands=(0.94,), loading_bands=(0.5, 0.9, 1.1),
                                     vmin=0.9, vmax=1.0, slots=False)
    assert [c["slots"] for c in seam] == [False, False] and (seam[0]["lo"], seam[0]["hi"]) == (0.9, 1.0)
    assert seam[1]["keep"].tolist() == [True, False, True, False, True, True]
    ar.check_report(acr, volt, load, [0, 0, 1, 0, -1], [0, 2, 5], [1.0, 0.0, 5.0, NAN, 2.0, 3.0], (0.94,), (0.5, 0.9, 1.1),
                    0.9, 1.0, slots=False)
    assert acr.daily_volt["n_nan"][0, 2] == 1 and acr.daily_volt["count"][0, 2] == 2


def test_probability_and_expected_slots():
    from revs_admm_amd.study import AcrossReport
    daily = ar.empty((2, 3))
    daily["count"] = [[4, 2, 0], [1, 1, 1]]
    daily["band_count"][..., 0] = [[1, 2, 0], [0, 1, 1]]
    daily["band_count"][..., 1] = [[4, 0, 0], [1, 0, 1]]
    expo = np.array([[6, 1, 0], [0, 24, 3]], np.int32)
    acr = AcrossReport(None, None, daily, None, expo, None, np.array([4, 1]), (0.92, 0.95), ())
    assert ar.same_numbers(acr.probability("volt", 0), [[0.25, 1.0, NAN], [0.0, 1.0, 1.0]])
    assert ar.same_numbers(acr.probability("volt", 1), [[1.0, 0.0, NAN], [1.0, 0.0, 1.0]])
    assert ar.same_numbers(acr.expected_slots("volt"), [[1.5, 0.5, NAN], [0.0, 24.0, 3.0]])
    with pytest.raises(ValueError, match="no loading records"):
        acr.probability("loading", 0)
    with pytest.raises(ValueError, match="'volt' or 'loading'"):
        acr.expected_slots("flow")


def test_ensemble_study_report_across(seam, monkeypatch):
    from network_worker import line_ratings
    from test_ensemble_report_host import _ensemble
    from revs_admm_amd import study
    w, load, P, e, Fake = _ensemble()
    seen = []
    monkeypatch.setattr(study, "native_study_device", ar.host_study_device(w.feeder, seen))
    rating, nodes = line_ratings(w)
    state = [t.clone() for t in (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)]
    with pytest.raises(ValueError, match="across=True.*pass groups"):
        e.study_report(across=True)
    with pytest.raises(ValueError, match="no scenario is in a group"):
        e.study_report(groups=[-1, -1, -1], across=True)
    assert Fake.calls == [] and seen == []                              # (refused before any launch)
    rep = e.study_report(groups=[1, 0, 1], rating=rating, nodes=nodes, arrays=True, across=True)
    assert seen == [dict(arrays=True, across=True, n_groups=2)] and len(Fake.calls) == 1 and len(seam) == 2
    assert (seam[0]["lo"], seam[0]["hi"]) == (e.vlow, e.vhigh)
    ar.check_report(rep.across, rep.volt, rep.loading, [1, 0, 1], nodes, rating, (0.92, 0.95, 0.98), (0.8, 1.0), e.vlow,
                    e.vhigh)
    assert e.study_report(groups=[1, 0, 1]).across is None and len(seam) == 2
    for a, b in zip(state, (e.P_est, e.P_sch, e.G, e.yd[0], e.diff)):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    from revs_admm_amd.ensemble import AdmmEnsemble
    with pytest.raises(NotImplementedError, match=r"voltages\(\)"):
        AdmmEnsemble.voltage(None)


def test_revs_study_across(host_revs, seam, monkeypatch):  # noqa: F811
    from revs_admm_amd import study
    fx, tariff, all_homes, dist, com, table, calls = host_revs
    monkeypatch.setattr(study, "native_study", ar.host_study)
    grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1, 2, 3), line_rating=table, arrays=True, bands=(0.95, 0.98))
    labels, rep = fx.study(tariff, all_homes, dist, com, across=True, **grid)
    assert rep.groups.tolist() == [0, 1] * 3 and len(seam) == 2
    acr = rep.across
    nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
    nodes = [nonsub.index(h) for h in com]
    assert int(seam[0]["keep"].sum()) == len(com) == 297 and int(seam[1]["keep"].sum()) == 1691
    assert acr.daily_volt.shape == (2, len(nonsub)) and acr.slot_volt.shape == (2, len(nonsub), 24)
    assert (acr.daily_volt["count"][:, nodes] == 3).all() and acr.daily_volt["count"].sum() == 2 * 3 * 297
    assert acr.bands_volt == (0.95, 0.98) and acr.group_sizes.tolist() == [3, 3]
    # exposure is the slots' violations summed, and the daily band count is bounded by the group
    assert np.array_equal(acr.exposure_volt, acr.slot_volt["n_violations"].sum(axis=2))
    assert np.array_equal(acr.exposure_loading, acr.slot_loading["n_violations"].sum(axis=2))
    prob = acr.probability("volt", 1)
    assert np.isnan(prob).sum() == 2 * (len(nonsub) - 297) and np.nanmax(prob) <= 1.0 and np.nanmax(prob) > 0.0
    ar.check_report(acr, rep.volt, rep.loading, rep.groups, nodes, seam[1]["keep"].astype(float), (0.95, 0.98), (0.8, 1.0),
                    0.95, 1.05)
    _, off = fx.study(tariff, all_homes, dist, com, **grid)
    assert off.across is None and len(seam) == 2
