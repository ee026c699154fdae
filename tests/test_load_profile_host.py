"""The load-profile report without a GPU: the numpy yard-stick (tests/profile_ref.py) on the stored data of the 121144
feeder -- its LOAD and the stored distributed and individual schedules, split by the stored EV homes -- anchored by
numbers read off the arrays themselves; the yard-stick's rules on awkward values; and every check of the Python entries
raising before the library is loaded."""
import math

import numpy as np
import pytest

import profile_ref as pr


def golden_profiles(z):
    """-> (g (3, n, T) float32: LOAD, distributed, individual; classes (3, n): 1 where the home owns an EV)."""
    g = np.stack([z["LOAD"], z["dis_a90_r4800_P_res"], z["ind_a90_r4800_P_res"]]).astype(np.float32)
    idx = {h: i for i, h in enumerate(z["res_id"])}
    ev = np.zeros(g.shape[1], np.int64)
    ev[[idx[h] for h in z["dis_a90_r4800_ev_homes"]]] = 1
    assert set(z["ind_a90_r4800_ev_homes"]) == set(z["dis_a90_r4800_ev_homes"])
    return g, np.tile(ev, (3, 1))


def test_golden_demand_curves(golden):
    z, _ = golden
    g, cls = golden_profiles(z)
    S, n, T = g.shape
    assert (S, n, T) == (3, 1126, 24) and cls[0].sum() == 267
    masks = pr.set_masks(cls, 2, S, n)
    x = g.astype(np.float64)
    for s in range(S):
        slot = pr.slot_records(g, masks, [s], 0.0)
        peak = pr.peak_records(g, masks, [s], 0.0)
        # anchors read off the arrays: counts per class, the aggregate's peak and its slot, a median
        assert [slot[q][0]["count"] for q in range(3)] == [n - 267, 267, n]
        agg = x[s].sum(axis=0)
        totals = np.array([slot[2][t]["total"] for t in range(T)])
        assert np.allclose(totals, agg, rtol=1e-12, atol=0)
        day = pr.day_record(totals, [slot[2][t]["count"] for t in range(T)], peak[2]["total"])
        assert day["peak_slot"] == int(np.argmax(agg)) and day["valley_slot"] == int(np.argmin(agg)) and day["slots"] == T
        assert math.isclose(day["peak"], agg.max(), rel_tol=1e-12) and math.isclose(day["energy"], agg.sum(), rel_tol=1e-12)
        assert math.isclose(day["load_factor"], agg.mean() / agg.max(), rel_tol=1e-12) and 0 < day["load_factor"] <= 1
        assert math.isclose(day["sum_peaks"], x[s].max(axis=1).sum(), rel_tol=1e-12) and day["diversity"] >= 1.0
        t = day["peak_slot"]
        assert slot[1][t]["box"]["median"] == np.median(x[s][cls[s] == 1][:, t])
        assert slot[2][t]["worst_index"] == int(np.argmax(x[s][:, t])) and slot[2][t]["worst_scenario"] == s
        # the sets add up
        for t in range(T):
            assert slot[0][t]["count"] + slot[1][t]["count"] == slot[2][t]["count"]
            assert math.isclose(slot[0][t]["total"] + slot[1][t]["total"], slot[2][t]["total"], rel_tol=1e-12)
    # the residences without an EV draw their base load under every schedule; the schedules move the EV homes' peak
    base = pr.slot_records(g, masks, [0], 0.0)
    dis = pr.slot_records(g, masks, [1], 0.0)
    for t in range(T):
        assert dis[0][t]["box"] == base[0][t]["box"] and dis[0][t]["total"] == base[0][t]["total"]
    assert max(dis[1][t]["total"] for t in range(T)) > max(base[1][t]["total"] for t in range(T))
    # pooled over the two schedules: the multiset of both
    pool = pr.slot_records(g, masks, [1, 2], 0.0)
    assert pool[2][5]["count"] == 2 * n and pool[2][5]["box"]["max"] == max(x[1][:, 5].max(), x[2][:, 5].max())


def test_yardstick_rules():
    nan, inf = np.nan, np.inf
    g = np.array([[[1.0, nan], [2.0, 5.0], [-0.0, 5.0], [inf, 1.0], [2.0, -inf], [-3.0, 4.0]]], np.float32)     # (1, 6, 2)
    cls = np.array([[0, 0, 1, 1, 2, 0]])                       # C = 2: the byte 2 leaves residence 4 out
    masks = pr.set_masks(cls, 2, 1, 6)
    assert [m[0].tolist() for m in masks] == [[1, 1, 0, 0, 0, 1], [0, 0, 1, 1, 0, 0], [1, 1, 1, 1, 0, 1]]
    slot = pr.slot_records(g, masks, [0], 1.0, index=[9, 8, 7, 6, 5, 4])
    r = slot[2][0]                                            # values 1, 2, -0.0, inf, -3 -> inf counts in n_nan
    assert (r["count"], r["n_nan"], r["n_above"], r["total"]) == (4, 1, 1, 0.0)
    assert r["box"]["min"] == -3.0 and r["box"]["max"] == 2.0 and r["worst_index"] == 8
    r = slot[1][0]                                            # -0.0 alone (inf left out): reported as +0.0
    assert r["count"] == 1 and r["box"]["min"] == 0.0 and not np.signbit(r["box"]["min"]) and r["n_above"] == 0
    r = slot[2][1]                                            # a tie for the largest: the lowest caller-side index
    assert (r["count"], r["n_nan"], r["box"]["max"], r["worst_index"]) == (4, 1, 5.0, 7)
    # peaks: a row with a value that is not finite gives a NaN, -inf included
    x = pr.peaks(g)
    assert x.dtype == np.float32 and np.isnan(x[0, [0, 3, 4]]).all() and x[0, [1, 2, 5]].tolist() == [5.0, 5.0, 4.0]
    p = pr.peak_records(g, masks, [0], 4.5)
    assert (p[0]["count"], p[0]["n_nan"], p[0]["n_above"], p[0]["total"]) == (2, 1, 1, 9.0)
    assert (p[1]["count"], p[1]["n_nan"]) == (1, 1) and (p[2]["count"], p[2]["n_nan"]) == (3, 2)
    # an empty class: NaN statistics, indices -1, counts 0
    e = pr.slot_records(g, pr.set_masks(np.array([[1, 1, 1, 1, 1, 1]]), 2, 1, 6), [0], 0.0)[0][0]
    assert (e["count"], e["n_nan"], e["n_above"], e["worst_index"], e["worst_scenario"]) == (0, 0, 0, -1, -1)
    assert e["box"] is None and np.isnan(e["total"])
    # no classes: one set of everybody
    assert len(pr.set_masks(None, 0, 1, 6)) == 1 and pr.set_masks(None, 0, 1, 6)[0].all()
    # a pool of one is the scenario's record
    g2 = np.concatenate([g, g[:, ::-1]])
    m2 = pr.set_masks(np.tile(cls, (2, 1)), 2, 2, 6)
    a, b = pr.slot_records(g2, m2, [1], 1.0), pr.slot_records(g2, m2, [1], 1.0)
    assert a == b and pr.slot_records(g2, m2, [0, 1], 1.0)[2][0]["count"] == 8


def test_day_formulas():
    d = pr.day_record([3.0, 7.0, 7.0, 1.0, 99.0, 1.0], [2, 2, 2, 2, 0, 1], 30.0)
    assert (d["peak"], d["peak_slot"], d["valley"], d["valley_slot"], d["slots"]) == (7.0, 1, 1.0, 3, 5)    # earliest on ties
    assert d["energy"] == 19.0 and d["load_factor"] == (19.0 / 5.0) / 7.0 and d["diversity"] == 30.0 / 7.0
    e = pr.day_record([1.0, 2.0], [0, 0], 5.0)
    assert e["slots"] == 0 and e["peak_slot"] == e["valley_slot"] == -1
    assert all(np.isnan(e[k]) for k in ("peak", "valley", "energy", "load_factor", "sum_peaks", "diversity"))
    pr.check_day(dict(d), d)
    with pytest.raises(AssertionError):
        pr.check_day(dict(d, energy=np.nextafter(19.0, 20.0)), d)


def test_value_errors_before_the_library_is_loaded(monkeypatch):
    from revs_admm_amd import _lib, load_profile as lp

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    ok = np.zeros((2, 5, 3), np.float32)
    with pytest.raises(ValueError, match="must be"):
        lp.load_profile_report(np.zeros(4))
    with pytest.raises(ValueError, match="scenarios outside"):
        lp.load_profile_report(np.zeros((4097, 1, 2)))
    with pytest.raises(ValueError, match="slots outside"):
        lp.load_profile_report(np.zeros((1, 2, 193)))
    with pytest.raises(ValueError, match="above is a NaN"):
        lp.load_profile_report(ok, above=float("nan"))
    with pytest.raises(ValueError, match="classes must be integers"):
        lp.load_profile_report(ok, classes=np.zeros((2, 4), int))
    with pytest.raises(ValueError, match="classes must be integers"):
        lp.load_profile_report(ok, classes=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="classes outside"):
        lp.load_profile_report(ok, classes=np.zeros((2, 5), int), n_classes=5)
    with pytest.raises(ValueError, match="without a class"):
        lp.load_profile_report(ok, n_classes=2)
    with pytest.raises(ValueError, match="names for"):
        lp.load_profile_report(ok, classes=np.zeros((2, 5), int), names=("a", "b"))
    with pytest.raises(ValueError):
        lp.load_profile_report(ok, groups=[0])                # one id per scenario
    with pytest.raises(ValueError):
        lp.load_profile_report(ok, groups=[0, -2])
    with pytest.raises(ValueError, match="group ids up to"):
        lp.load_profile_report(ok, groups=[0, 2])
    with pytest.raises(ValueError, match="float32 tensor"):
        lp.load_profile_report_device(ok)
    import torch
    with pytest.raises(ValueError, match="runs on the GPU"):
        lp.load_profile_report_device(torch.zeros(5, 2, 3))
    with pytest.raises(ValueError, match="not contiguous"):
        lp.load_profile_report_device(torch.zeros(5, 2, 6)[:, :, ::2])
    with pytest.raises(ValueError, match="index must be"):
        lp.load_profile_report_device(torch.zeros(5, 2, 3), index=[0, 1, 2])
    # what the checks return
    cls, C, sets, gid, G, above, index = lp.check_profile_args(2, 5, 3, [[0, 1, 2, 7, -1]] * 2, None, [0, 0], 0.5,
                                                               index=[4, 3, 2, 1, 0], names=None)
    assert cls.tolist() == [[0, 1, 2, 255, 255]] * 2 and C == 3 and sets == ("class 0", "class 1", "class 2", "all")
    assert gid.tolist() == [0, 0] and G == 1 and above == 0.5 and index.dtype == np.int32
    assert lp.check_profile_args(1, 5, 3, None, None, None, -np.inf)[:3] == (None, 0, ("all",))


def test_report_helpers():
    from revs_admm_amd._lib import BILL_DTYPE, PROFILE_DAY_DTYPE
    from revs_admm_amd.load_profile import LoadProfileReport
    slot = np.zeros((2, 1, 3), BILL_DTYPE)
    slot["total"], slot["count"] = [[[2.0, 4.0, 6.0]], [[1.0, np.nan, 3.0]]], [[[2, 2, 2]], [[1, 0, 3]]]
    day = np.zeros((2, 1), PROFILE_DAY_DTYPE)
    day["peak"] = [[6.0], [3.0]]
    rep = LoadProfileReport(slot, np.zeros((2, 1), BILL_DTYPE), day, np.zeros((1, 1, 3), BILL_DTYPE),
                            np.zeros((1, 1), BILL_DTYPE), ("all",), np.array([0, 0]), 1, 0.0)
    assert rep.aggregate().tolist()[0] == [[2.0, 4.0, 6.0]] and rep.mean()[0, 0].tolist() == [1.0, 2.0, 3.0]
    assert np.isnan(rep.mean()[1, 0, 1]) and rep.mean()[1, 0, 2] == 1.0
    other = LoadProfileReport(slot, rep.peak, day.copy(), rep.pooled_slot, rep.pooled_peak, ("all",), rep.groups, 1, 0.0)
    other.day["peak"] = [[4.0], [3.0]]
    assert rep.peak_change(other).tolist() == [[50.0], [0.0]]
    assert rep.group_day_mean()["peak"].tolist() == [[4.5]]
