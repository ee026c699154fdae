"""The charging report without a GPU: the numpy yard-stick (tests/charge_ref.py) on the stored results of the 121144
feeder -- the distributed and the individual schedules' charger power -- anchored by numbers read off the arrays
themselves; the yard-stick's rules on awkward rows; and every check of the Python entries raising before the library is
loaded."""
import numpy as np
import pytest

import charge_ref as cr

# The stored charger power is an LP solver's: "off" is rounding dust of either sign around 1e-15 and "on" is the rating.
# The anchors are counts of slots at the rating, so the threshold sits between the two.
ON_FRAC = 0.5


def golden_case(z, tag):
    from revs_admm_amd.engine import pack_homes
    p = z[tag + "_P_ev"].astype(np.float32)
    assert p.shape == (267, 24) and np.abs(z[tag + "_P_ev"][z[tag + "_P_ev"] < 1.0]).max() < 1e-12
    homes = pack_homes(np.ones(267, bool), 4.8, 20.0, 0.2, 11, 23)
    return p[None], homes[None]


def test_golden_distributed_schedule_is_staggered(golden):
    z, _ = golden
    p, homes = golden_case(z, "dis_a90_r4800")
    r = cr.report(p, homes, z["tariff_shift6"], ON_FRAC)
    assert (r.row["n_on"] == 3).all() and (r.row["n_full"] == 3).all()
    assert r.hist[0, 0].tolist() == [0, 0, 0, 267] + [0] * 21
    assert r.hist[0, 2, :4].tolist() == [0, 119, 119, 29] and r.hist[0, 2].sum() == 267
    assert r.slot["n_on"][0, 11:23].tolist() == [8, 6, 7, 6, 7, 17, 45, 136, 113, 203, 191, 62]
    assert r.slot["n_on"][0, :11].sum() == 0 and r.slot["n_on"][0, 23] == 0
    assert int(r.day["peak_on"][0]) == 203 and int(r.day["peak_on_slot"][0]) == 20
    assert int(r.day["n_outside"][0]) == 0 and (r.row["n_outside"] == 0).all()
    assert (r.row["first_on"] >= 11).all() and (r.row["last_on"] < 23).all()
    # the first-on slots spread over slots 11 .. 20
    first = np.bincount(r.row["first_on"][0], minlength=24)
    assert first[11:21].tolist() == [8, 6, 5, 2, 5, 9, 37, 100, 70, 25] and first.sum() == 267
    assert r.hist[0, 1, :10].tolist() == first[11:21].tolist()          # wait = first_on - 11
    assert int(r.day["n_interrupted"][0]) == 119 + 29 and int(r.day["n_never"][0]) == 0 and int(r.day["n_ev"][0]) == 267
    assert r.day["coincidence"][0] == 203 / 267
    assert (r.slot["n_plugged"][0] == np.where((np.arange(24) >= 11) & (np.arange(24) < 23), 267, 0)).all()
    assert r.slot["n_starts"][0].sum() == 119 + 2 * 119 + 3 * 29
    _soc_and_energy(z, "dis_a90_r4800", p, r)


def test_golden_individual_schedule_switches_everybody_on_together(golden):
    z, _ = golden
    p, homes = golden_case(z, "ind_a90_r4800")
    r = cr.report(p, homes, z["tariff_shift6"], ON_FRAC)
    assert r.slot["n_on"][0].tolist() == [0] * 20 + [267] * 3 + [0]
    assert r.day["coincidence"][0] == 1.0 and int(r.day["peak_on"][0]) == 267 and int(r.day["peak_on_slot"][0]) == 20
    assert (r.row["sessions"] == 1).all() and r.hist[0, 2, 1] == 267 and int(r.day["n_interrupted"][0]) == 0
    assert (r.row["wait"] == 9).all() and r.hist[0, 1, 9] == 267
    assert r.slot["n_starts"][0].tolist() == [0] * 20 + [267] + [0] * 3
    _soc_and_energy(z, "ind_a90_r4800", p, r)


def _soc_and_energy(z, tag, p, r):
    soc = z[tag + "_SOC"][:, -1]
    assert np.abs(soc - 0.92).max() < 1e-9
    # float rounding: the float32 of the rating (3 slots of it over 20 kWh) and of the result
    assert np.abs(r.row["soc_end"][0].astype(np.float64) - soc).max() <= 4 * 2.0 ** -24
    assert (r.row["flags"] == 1).all() and int(r.day["n_under"][0]) == 0
    assert r.keep.all() and not np.isnan(r.val).any()
    assert np.allclose(r.row["energy"][0], 3 * 4.8, rtol=1e-6)
    cost = (z["tariff_shift6"][None, :] * p[0].astype(np.float64)).sum(1)
    assert np.allclose(r.row["cost"][0], cost, rtol=1e-12) and np.isclose(r.day["cost"][0], cost.sum(), rtol=1e-12)
    assert np.isclose(r.day["energy"][0], p.astype(np.float64).sum(), rtol=1e-12)
    assert np.isclose(r.day["peak_power"][0], p[0].astype(np.float64).sum(0).max(), rtol=1e-12)


@pytest.mark.parametrize("T", [1, 5, 24])
@pytest.mark.parametrize("on_frac", [0.0, 0.5])
def test_awkward_rows(T, on_frac):
    tol = 1e-6
    rec, p = cr.awkward_rows(T, on_frac, tol)
    k = {name: i for i, name in enumerate(cr.AWKWARD)}
    tariff = np.linspace(0.05, 0.3, T)
    r = cr.report(p[None], rec[None], tariff, on_frac, tol)
    row = {f: v[0] for f, v in r.row.items()}
    ws = min(1, T - 1)
    assert row["first_on"][k["on_at_0"]] == 0 and row["wait"][k["on_at_0"]] == -ws and row["sessions"][k["on_at_0"]] == 1
    assert row["n_outside"][k["on_at_0"]] == (1 if ws > 0 else 0)
    assert row["last_on"][k["on_at_last"]] == T - 1 and row["first_on"][k["on_at_last"]] == T - 1
    assert row["sessions"][k["alternating"]] == (T + 1) // 2 == row["n_on"][k["alternating"]]
    assert row["n_full"][k["exactly_rating"]] == 1 and row["n_on"][k["exactly_rating"]] == 1
    assert row["n_full"][k["just_below_rating"]] == 0 and row["n_on"][k["just_below_rating"]] == 1
    assert row["n_on"][k["at_threshold"]] == 0 and row["first_on"][k["at_threshold"]] == -1 and row["wait"][k["at_threshold"]] == -1
    assert row["n_on"][k["just_above_threshold"]] == 1
    assert row["n_on"][k["negative"]] == 1 and row["energy"][k["negative"]] < 0 or T == 1
    # a NaN slot is off and sets bit 2; the row is not kept and its values are NaN
    i = k["nan"]
    assert row["flags"][i] & 4 and np.isnan(row["energy"][i]) and r.keep[0, i] == 0 and np.isnan(r.val[:, 0, i]).all()
    assert row["n_on"][i] == (1 if T > 1 else 0)
    assert row["flags"][k["pos_inf"]] & 4 and row["n_on"][k["pos_inf"]] == 1 and row["n_full"][k["pos_inf"]] == 1
    assert row["flags"][k["neg_inf"]] & 4 and row["n_on"][k["neg_inf"]] == 0
    # windows: clamped into 0..T; an empty window (end < start) puts every on slot outside
    assert row["wait"][k["start_below_0"]] == 0 and row["n_outside"][k["start_below_0"]] == 0
    assert row["n_outside"][k["end_beyond_T"]] == ws
    assert row["n_outside"][k["end_before_start"]] == T and row["wait"][k["end_before_start"]] == -(T - 1)
    i = k["no_ev_with_power"]
    assert all(row[f][i] == 0 for f in ("energy", "cost", "soc_end", "n_on", "n_full", "sessions", "n_outside", "flags"))
    assert row["first_on"][i] == row["last_on"][i] == row["wait"][i] == -1 and r.keep[0, i] == 0
    assert row["flags"][k["short_by_more"]] == 3 and row["flags"][k["short_by_less"]] == 1
    # histograms leave negative waits and chargers that are never on out
    counted = (row["flags"] & 1 == 1) & (row["first_on"] >= 0) & (row["wait"] >= 0)
    assert r.hist[0, 1].sum() == counted.sum() < (row["flags"] & 1).sum() == r.hist[0, 0].sum() == r.hist[0, 2].sum()
    assert int(r.day["n_ev"][0]) == len(cr.AWKWARD) - 1
    # without a tariff every cost is a NaN, nothing else moves
    q = cr.report(p[None], rec[None], None, on_frac, tol)
    assert np.isnan(q.row["cost"][0][row["flags"] & 1 == 1]).all() and np.isnan(q.day["cost"][0]) and np.isnan(q.val[1]).all()
    assert q.row["cost"][0, k["no_ev_with_power"]] == 0
    assert q.val[0].tobytes() == r.val[0].tobytes() and (q.hist == r.hist).all()


def test_a_scenario_without_an_ev():
    rng = np.random.default_rng(3)
    p, homes = cr.random_case(rng, 3, 40, 7)
    r = cr.report(p, homes, np.ones(7))
    assert int(r.day["n_ev"][1]) == 0 and np.isnan(r.day["coincidence"][1])
    assert int(r.day["peak_on_slot"][1]) == -1 and int(r.day["peak_power_slot"][1]) == -1 and r.day["peak_power"][1] == 0.0
    assert not r.hist[1].any() and not r.keep[1].any() and np.isnan(r.val[:, 1]).all()
    assert not r.slot["n_on"][1].any() and (r.slot["power"][1] == 0).all() and r.day["cost"][1] == 0.0


def test_python_checks_raise_before_the_library_is_loaded(monkeypatch):
    import torch
    from revs_admm_amd import _lib, charging as ch
    from revs_admm_amd._lib import HOME_DTYPE

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    ok = dict(S=2, n=8, T=5, tariff=np.ones(5), groups=[0, -1], on_frac=0.0, short_tol=1e-6)
    ch.check_charge_args(**ok)
    for bad, match in ((dict(S=0), "scenarios"), (dict(S=4097), "scenarios"), (dict(T=0), "slots"), (dict(T=193), "slots"),
                       (dict(n=0), "rows"), (dict(n=2 ** 30), "rows"), (dict(tariff=np.ones(4)), "one price per slot"),
                       (dict(on_frac=-1.0), "on_frac"), (dict(on_frac=float("nan")), "on_frac"),
                       (dict(short_tol=-1e-9), "short_tol"), (dict(short_tol=float("nan")), "short_tol"),
                       (dict(groups=[0, 1, 2]), "groups"), (dict(groups=[-2, 0]), "groups"), (dict(groups=[0, 5]), "group ids"),
                       (dict(index=np.arange(7)), "index"), (dict(index=-np.arange(8)), "index")):
        with pytest.raises(ValueError, match=match):
            ch.check_charge_args(**{**ok, **bad})
    p = np.zeros((2, 8, 5), np.float32)
    rec = np.zeros((2, 8), HOME_DTYPE)
    for args, match in (((np.zeros(5), rec), "p must be"), ((p, rec[:, :7]), "records must be"),
                        ((p, np.zeros((2, 8))), "records must be"), ((np.zeros((2, 8, 0)), rec), "p must be")):
        with pytest.raises(ValueError, match=match):
            ch.charging_report(*args)
    with pytest.raises(ValueError, match="on_frac"):
        ch.charging_report(p, rec, on_frac=-1)
    with pytest.raises(ValueError, match="one price per slot"):
        ch.charging_report(p, rec, tariff=np.ones(3))
    homes = torch.zeros(2 * 8 * 32, dtype=torch.uint8)
    for t, match in ((torch.zeros(8, 2, 5, dtype=torch.float64), "float32 tensor"), (torch.zeros(8, 5)[:, ::2], "slots are not"),
                     (torch.zeros(0, 5), "empty"), (np.zeros((8, 5), np.float32), "float32 tensor")):
        with pytest.raises(ValueError, match=match):
            ch.charging_report_device(t, homes)
    with pytest.raises(ValueError, match="runs on the GPU"):
        ch.charging_report_device(torch.zeros(8, 2, 5), homes)
    with pytest.raises(ValueError, match="rows must be"):
        ch.charging_report_device(torch.zeros(8, 2, 5), homes, rows="host")


def test_report_helpers():
    from revs_admm_amd import _lib
    from revs_admm_amd.charging import POOLED_SLOT_DTYPE, ChargingReport
    S, T = 2, 4
    slot = np.zeros((S, T), _lib.CHARGE_SLOT_DTYPE)
    slot["n_ev"], slot["n_on"] = [[4] * T, [0] * T], [[0, 1, 4, 2], [0] * T]
    day = np.zeros(S, _lib.CHARGE_DAY_DTYPE)
    day["peak_on"], day["peak_power"], day["cost"] = [4, 0], [19.2, 0.0], [3.0, 0.0]
    box = lambda tot, cnt: np.array([(0,) * 7 + (tot, 0, cnt, 0, 0, 0, -1, -1)] * S, _lib.BILL_DTYPE)
    mk = lambda w: ChargingReport(None, slot, day, np.zeros((S, 3, T + 1), np.int32), box(0, 4), box(0, 4), box(0, 4), w,
                                  *(np.zeros(0, _lib.BILL_DTYPE),) * 4, np.zeros((0, T), POOLED_SLOT_DTYPE),
                                  np.zeros((0, 3, T + 1), np.int64), np.full(S, -1), 0, 0.0, 1e-6)
    a, b = mk(box(8.0, 4)), mk(box(2.0, 4))
    assert a.on_curve().tolist() == slot["n_on"].tolist()
    c = a.coincidence()
    assert c[0].tolist() == [0.0, 0.25, 1.0, 0.5] and np.isnan(c[1]).all()
    d = a.compare(b)
    assert d["wait"].tolist() == [1.5, 1.5] and d["peak_on"].tolist() == [0, 0] and d["cost"].tolist() == [0.0, 0.0]
