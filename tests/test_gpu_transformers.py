"""The transformer report on the GPU (revs_xf_report; transformers.report_for_rows, AdmmEngine.transformer_report,
AdmmEnsemble.transformer_reports, REVS.study(transformers=)) against tests/xf_ref.py.

Bit for bit: load, ratio, summary_ratio and the day record's peak_ratio / peak_ratio_slot / energy_kwh / n_over_slots
against restate(); summary_hot, the rest of the day record and the fleet record against restate() fed the kernel's own
hot_spot and faa (the loss tests' contract() idiom); the summaries by check_summary's rules (== for order statistics and
counts, <= 2 ulp for the interpolated quartiles).  Within a derived bound: top_oil, hot_spot and faa against restate()
through xf_ref.propagated_bounds at E = 16 ulp for each pow and exp -- the OpenCL full-profile bound for pow, taken
because no documented bound of the HIP device library's double pow and exp was at hand; the measured maxima are printed
beside the bounds."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import xf_ref as xr
from test_gpu_network import ulps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ULP = 16.0
ARRAYS = ("load", "ratio", "top_oil", "hot_spot", "faa")
RECORDS = ("summary_ratio", "summary_hot", "xf_day", "fleet")
DAY_FROM_LOAD = ("peak_ratio", "energy_kwh")
DAY_FROM_HOT = ("peak_hot", "age_hours", "lol_percent", "feqa")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def bits(got, want, what):
    """Equal as doubles including the NaNs' places, and equal in bytes where they are no NaNs."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and same(got, want), (what, got, want)
    ok = ~np.isnan(want)
    assert got[ok].tobytes() == want[ok].tobytes(), what


def check_summary(rec, ref, what):
    for t, r in enumerate(ref):
        g = rec[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"]), (what, t, g, r)
        if r["count"] == 0:
            assert np.isnan(g["min"]) and np.isnan(g["median"]) and np.isnan(g["worst_value"]) and g["n_fliers"] == 0
            continue
        box = r["box"]
        for k in ("min", "max", "whisker_lo", "whisker_hi"):
            assert g[k] == box[k], (what, t, k, g[k], box[k])
        assert g["worst_value"] == r["worst_value"]
        for k in ("q1", "median", "q3"):
            assert g[k] == box[k] or ulps(g[k], box[k]) <= 2, (what, t, k, g[k], box[k])
        assert g["n_fliers"] == box["n_fliers"], (what, t, g, box)


def check_report(rep, g, xf_ptr, xf_rows, rated_kw, ambient, model=None, slot_hours=None, substeps=1, initial="cyclic",
                 over_ratio=1.0, hot_limit=110.0, tag=""):
    """One scenario's TransformerReport against the restatement -> (restate() on its own arrays, the measured maxima)."""
    from revs_admm_amd.transformers import ThermalModel
    model = ThermalModel() if model is None else model
    T = g.shape[1]
    hours = 24.0 / T if slot_hours is None else slot_hours
    mdl = {k: getattr(model, k) for k in xr.MODEL}
    d_to, d_w = model.decays(hours, substeps)
    cyc, (to0, w0) = (1, (0.0, 0.0)) if initial == "cyclic" else (0, initial)
    kw = dict(mdl=mdl, slot_hours=hours, q=substeps, decay_to=d_to, decay_w=d_w, cyclic=cyc, to0=to0, w0=w0,
              over_ratio=over_ratio, hot_limit=hot_limit)
    r = xr.restate(g, xf_ptr, xf_rows, rated_kw, ambient, **kw)
    bad = r["bad"]
    # ---- bit for bit: what depends on the grouped sums alone
    bits(rep.load, r["load"], "load")
    bits(rep.ratio, r["ratio"], "ratio")
    check_summary(rep.summary_ratio, r["summary_ratio"], "ratio")
    for k in DAY_FROM_LOAD:
        bits(rep.xf_day[k], r["day"][k], k)
    assert same(rep.xf_day["peak_ratio_slot"], r["day"]["peak_ratio_slot"]) and same(rep.xf_day["n_over_slots"], r["day"]["n_over_slots"])
    # ---- within the derived bound: the thermal arrays
    b_top, b_hot, b_faa = xr.propagated_bounds(r, ambient, mdl, substeps, d_to, d_w, cyc, E_ULP)
    worst = {}
    for name, got, want, b in (("top_oil", rep.top_oil, r["top_oil"], b_top), ("hot_spot", rep.hot_spot, r["hot"], b_hot),
                               ("faa", rep.faa, r["faa"], b_faa)):
        assert np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any(), name
        if (~bad).any():
            err = np.abs(got[~bad] - want[~bad])
            worst[name] = (float(err.max()), float(b[~bad][np.unravel_index(err.argmax(), err.shape)]),
                           float((err / b[~bad]).max()))
            assert (err <= b[~bad]).all(), (name, worst[name])
    if worst:
        print(f"{tag} K={len(rated_kw)} T={T} q={substeps} {'cyclic' if cyc else 'given'}: " +
              ", ".join(f"{k} err {v[0]:.2e} (bound there {v[1]:.2e}, largest err/bound {v[2]:.3f})" for k, v in worst.items()))
    # ---- bit for bit on the kernel's own hot_spot and faa: the records behind them
    c = xr.restate(g, xf_ptr, xf_rows, rated_kw, ambient, hot=rep.hot_spot, faa=rep.faa, **kw)
    check_summary(rep.summary_hot, c["summary_hot"], "hot")
    for k in DAY_FROM_HOT:
        bits(rep.xf_day[k], c["day"][k], k)
    assert same(rep.xf_day["peak_hot_slot"], c["day"]["peak_hot_slot"]) and same(rep.xf_day["n_hot_slots"], c["day"]["n_hot_slots"])
    f = c["fleet"]
    for k in ("n_xf", "n_nan", "n_overloaded", "n_hot", "n_aging"):
        assert int(rep.fleet[k]) == f[k], (k, rep.fleet[k], f[k])
    for k in ("lol_sum", "lol_max", "energy_kwh", "feqa_mean", "top_lol"):
        bits(rep.fleet[k], f[k], "fleet " + k)
    assert same(rep.fleet["top_index"], f["top_index"]), (rep.fleet["top_index"], f["top_index"])
    assert (rep.fleet["reserved"] == 0).all()
    return c, worst


def native(g, xf_ptr, xf_rows, rated_kw, ambient, **kw):
    """revs_xf_report through its one caller, on a CSR given as it is (no validation of the rows: the raw ABI's view)."""
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.transformers import native_transformers_device
    dev = torch.device("cuda:0")
    g3 = torch.from_numpy(np.array(g if g.ndim == 3 else g[None], np.float64)).to(dev)       # (a copy: the cases are read-only)
    reps = native_transformers_device(_lib.load(), dev, torch.cuda.current_stream(dev).cuda_stream, g3, xf_ptr, xf_rows,
                                      rated_kw, ambient, **kw)
    return reps if g.ndim == 3 else reps[0]


@functools.lru_cache(maxsize=None)
def fleet_case(K, T):
    """K transformers with 0 - 14 rows each (transformer 1 empty where there is one, the last with at least one row), rows
    ascending within a transformer but scattered over g, five rows owned by nobody, ratings off the ladder, loads with
    ratios from 0 to about 3 (a tenth of the rows exporting).  T = 3 carries the bad transformers that fit: a NaN member
    in slot 1 of transformer 0; with K >= 3 rated_kw = 0 at K // 2; with K >= 2 a row index of m in the last list."""
    rng = np.random.default_rng(1000 * K + T)
    counts = rng.integers(0, 15, K)
    counts[0], counts[-1] = max(counts[0], 2), max(counts[-1], 1)
    if K > 2:
        counts[1] = 0
    nnz = int(counts.sum())
    m = nnz + 5
    perm = rng.permutation(m)[:nnz]
    cuts = np.concatenate([[0], np.cumsum(counts)])
    members = [np.sort(perm[cuts[k]:cuts[k + 1]]).tolist() for k in range(K)]
    xf_ptr, xf_rows = xr.csr(members)
    rated = rng.choice([5.0, 10.0, 15.0, 25.0, 37.5], K) * 0.95
    g = rng.uniform(0.0, 1.0, (m, T))
    for k in range(K):
        if counts[k]:
            g[members[k]] *= rated[k] * rng.uniform(0.0, 3.0, (1, T)) / g[members[k]].sum(axis=0)
    g[rng.random(m) < 0.1] *= -0.3
    ambient = 20.0 + 10.0 * rng.random(T)
    if T == 3:
        g[members[0][1], 1] = np.nan
        if K >= 3:
            rated[K // 2] = 0.0
        if K >= 2:
            xf_rows = xf_rows.copy()
            xf_rows[-1] = m
    for a in (g, xf_ptr, xf_rows, rated, ambient):
        a.setflags(write=False)
    return g, xf_ptr, xf_rows, rated, ambient


def clear_limit(r, hot_limit=110.0):
    """A hot_limit that no restated hot-spot lies within 1e-6 K of (moved up in steps of 1e-3 K where one does); no
    restated feqa within 1e-9 of 1."""
    hot = r["hot"][~np.isnan(r["hot"])]
    while hot.size and np.abs(hot - hot_limit).min() <= 1e-6:
        hot_limit += 1e-3
    feqa = r["day"]["feqa"][~np.isnan(r["day"]["feqa"])]
    assert not feqa.size or np.abs(feqa - 1.0).min() > 1e-9
    assert not hot.size or np.abs(hot - hot_limit).min() > 1e-6
    return hot_limit


@pytest.mark.parametrize("initial", ["cyclic", (20.0, 3.0)], ids=["cyclic", "given"])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("T", [1, 3, 24])
@pytest.mark.parametrize("K", [1, 64, 65, 1000])
def test_every_shape_matches_the_restatement(gpu_lib, K, T, substeps, initial):
    """One transformer, four full tiles, one transformer beyond them, 63 tiles; one slot, three (with the bad
    transformers) and a day; one and four sub-steps; both starts."""
    from revs_admm_amd.transformers import ThermalModel
    g, xf_ptr, xf_rows, rated, ambient = fleet_case(K, T)
    hours = 24.0 / T if T > 1 else 1.0
    d_to, d_w = ThermalModel().decays(hours, substeps)
    cyc, (to0, w0) = (1, (0.0, 0.0)) if initial == "cyclic" else (0, initial)
    pre = xr.restate(g, xf_ptr, xf_rows, rated, ambient, slot_hours=hours, q=substeps, decay_to=d_to, decay_w=d_w, cyclic=cyc,
                     to0=to0, w0=w0)
    hot_limit = clear_limit(pre)                                  # (before any launch)
    kw = dict(slot_hours=hours, substeps=substeps, initial=initial, over_ratio=1.0, hot_limit=hot_limit)
    rep = native(g, xf_ptr, xf_rows, rated, ambient, **kw)
    c, _ = check_report(rep, g, xf_ptr, xf_rows, rated, ambient, tag="shapes", **kw)
    want_bad = 0 if T != 3 else min(K, 3)
    assert c["bad"].sum() == want_bad == rep.fleet["n_nan"] and rep.fleet["n_xf"] == K
    if T == 3:
        assert (rep.summary_hot["n_nan"] == want_bad).all() and np.isnan(rep.load[0, 1]) and not np.isnan(rep.load[0, 0])
        if K >= 3:
            assert np.isinf(rep.ratio[K // 2]).any() and np.isnan(rep.xf_day["energy_kwh"][K // 2])
            assert rep.xf_day["n_over_slots"][K // 2] == 0 and rep.xf_day["peak_hot_slot"][K // 2] == -1
    if K > 2:
        assert (rep.load[1] == 0).all() and not np.isnan(rep.hot_spot[1]).any()          # the empty transformer is valid
    if K >= 64 and T == 24:
        assert rep.fleet["n_overloaded"] > 0 and rep.fleet["n_aging"] > 0 and rep.ratio[~c["bad"]].max() > 2.0
        assert len(rep.top_transformers) == 8 and set(rep.overloaded) == set(np.flatnonzero(rep.xf_day["n_over_slots"] > 0))


@pytest.mark.parametrize("T", [96, 192])
def test_long_days_match_the_restatement(gpu_lib, T):
    """The study's T = 96 and the largest T, where a workgroup's staging takes 102 KB of LDS: 70 transformers (five
    tiles, the last one partial), substeps = 2."""
    g, xf_ptr, xf_rows, rated, ambient = fleet_case(70, T)
    kw = dict(slot_hours=24.0 / T, substeps=2, hot_limit=120.0)
    rep = native(g, xf_ptr, xf_rows, rated, ambient, **kw)
    c, _ = check_report(rep, g, xf_ptr, xf_rows, rated, ambient, tag="long", **kw)
    assert not c["bad"].any() and rep.fleet["n_xf"] == 70 and rep.fleet["n_overloaded"] > 0


def test_scenario_grid_outputs_alone_and_records_only(gpu_lib):
    """S = 3: each scenario's slice holds the bytes of the S = 1 call.  Each output alone, every other one NULL (the
    arrays without any scratch), holds the bytes of the full call.  arrays=False gives the same records."""
    import ctypes as C
    import torch
    from revs_admm_amd import _lib
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.transformers import ThermalModel
    g, xf_ptr, xf_rows, rated, ambient = fleet_case(65, 24)
    gs = np.stack([g, g * 0.5, g[:, ::-1].copy()])
    kw = dict(slot_hours=0.5, substeps=2, hot_limit=95.0)
    reps = native(gs, xf_ptr, xf_rows, rated, ambient, **kw)
    only = native(gs, xf_ptr, xf_rows, rated, ambient, arrays=False, **kw)
    for s in range(3):
        one = native(gs[s], xf_ptr, xf_rows, rated, ambient, **kw)
        check_report(reps[s], gs[s], xf_ptr, xf_rows, rated, ambient, tag=f"grid s={s}", **kw)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert only[s].load is None and only[s].faa is None
        for k in RECORDS:
            assert getattr(only[s], k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
    lib, dev = gpu_lib, torch.device("cuda:0")
    S, (m, T), K = 3, g.shape, 65
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_g, d_ptr, d_rows, d_rated, d_amb = up(gs), up(xf_ptr), up(xf_rows), up(rated), up(ambient)
    mdl = ThermalModel()
    d_to, d_w = mdl.decays(0.5, 2)
    scratch = torch.empty(lib.revs_xf_report_scratch(S, T, K) // 8, dtype=torch.float64, device=dev)
    stack = lambda k: np.stack([getattr(r, k) for r in reps])
    wants = [stack(k) for k in ARRAYS + RECORDS]
    sizes = [S * K * T * 8] * 5 + [S * T * SUMMARY_DTYPE.itemsize] * 2 + [S * K * 64, S * 160]
    for k in range(9):
        outs = [None] * 9
        outs[k] = torch.zeros(sizes[k], dtype=torch.uint8, device=dev)
        rc = lib.revs_xf_report(S, m, T, K, len(xf_rows), d_g.data_ptr(), d_ptr.data_ptr(), d_rows.data_ptr(),
                                d_rated.data_ptr(), d_amb.data_ptr(), C.byref(mdl.struct()), 0.5, 2, d_to, d_w, 1, 0.0, 0.0,
                                1.0, 95.0, *[None if o is None else o.data_ptr() for o in outs],
                                scratch.data_ptr() if k in (5, 6, 8) else None, None)
        assert rc == 0, lib.revs_last_error()
        torch.cuda.synchronize()
        assert outs[k].cpu().numpy().tobytes() == np.ascontiguousarray(wants[k]).tobytes(), k
    assert _lib.XF_DAY_DTYPE.itemsize == 64


def test_ties_and_fewer_than_eight_transformers(gpu_lib):
    """Twelve identical transformers: every value ties -- worst_index 0, the top 8 are 0..7 in order.  Five transformers:
    the top 8 end in -1 / NaN."""
    T = 4
    g = np.tile(np.array([[3.0, 6.0, 12.0, 6.0]]), (12, 1))
    xf_ptr, xf_rows = xr.csr([[k] for k in range(12)])
    rep = native(g, xf_ptr, xf_rows, np.full(12, 9.5), np.full(T, 30.0), slot_hours=6.0)
    check_report(rep, g, xf_ptr, xf_rows, np.full(12, 9.5), np.full(T, 30.0), slot_hours=6.0, tag="ties")
    assert (rep.summary_ratio["worst_index"] == 0).all() and (rep.summary_hot["worst_index"] == 0).all()
    assert rep.fleet["top_index"].tolist() == list(range(8)) and len(set(rep.fleet["top_lol"].tolist())) == 1
    assert len(set(rep.hot_spot[:, 2].tolist())) == 1 and (rep.summary_hot["n_fliers"] == 0).all()
    assert (rep.xf_day["peak_ratio_slot"] == 2).all() and rep.fleet["n_overloaded"] == 12
    g5 = g[:5] * np.array([[1.0], [2.0], [2.0], [0.5], [1.0]])
    xf_ptr, xf_rows = xr.csr([[k] for k in range(5)])
    rep = native(g5, xf_ptr, xf_rows, np.full(5, 9.5), np.full(T, 30.0), slot_hours=6.0)
    check_report(rep, g5, xf_ptr, xf_rows, np.full(5, 9.5), np.full(T, 30.0), slot_hours=6.0, tag="five")
    assert rep.fleet["top_index"].tolist() == [1, 2, 0, 4, 3, -1, -1, -1] and np.isnan(rep.fleet["top_lol"][5:]).all()
    assert rep.top_transformers[0][0] == 1 and len(rep.top_transformers) == 5


@functools.lru_cache(maxsize=None)
def golden_fleet():
    """Owners from the golden graph's labels (residence rows), ratings from size_ratings of the base load."""
    from oracle import revs_oracle as ro
    from test_network_host import golden_graph
    from revs_admm_amd.transformers import build_csr, rows_by_transformer, size_ratings
    golden = ro.load_golden(os.path.join(HERE, "golden", "revs_121144.npz"))
    xf_nodes, xf_of = rows_by_transformer(golden_graph(golden))
    load = np.asarray(golden[0]["LOAD"], np.float64)
    base = np.zeros((len(xf_nodes), load.shape[1]))
    np.add.at(base, xf_of, load)
    kva = size_ratings(base.max(axis=1), pf=0.95)
    return golden[0], xf_of, kva, build_csr(xf_of, len(xf_of), len(kva))


def test_golden_feeder_under_the_stored_schedules(gpu_lib):
    """The 121144 feeder's 462 transformers, T = 24, under the base load and the stored individual and distributed
    schedules: each equals the restatement.  Sized from the base load no transformer is above its rating under it; under
    the individual schedule some are.  (Which schedule ages the fleet less is printed, not asserted.)"""
    from revs_admm_amd.transformers import report_for_rows
    z, xf_of, kva, (xf_ptr, xf_rows) = golden_fleet()
    ambient = np.full(24, 30.0)
    lol = {}
    for tag in ("LOAD", "ind_a90_r4800_P_res", "dis_a90_r4800_P_res"):
        p = np.asarray(z[tag], np.float64)
        rep = report_for_rows(p, xf_of, kva, slot_hours=1.0)
        check_report(rep, p, xf_ptr, xf_rows, kva * 0.95, ambient, slot_hours=1.0, tag=tag)
        assert rep.fleet["n_nan"] == 0 and rep.fleet["n_xf"] == 462
        lol[tag] = float(rep.fleet["lol_sum"])
        print(f"{tag}: {rep.fleet['n_overloaded']} overloaded, highest ratio {rep.xf_day['peak_ratio'].max():.2f}, "
              f"{rep.fleet['n_hot']} above 110 C, fleet loss of life {lol[tag]:.4f} % (sum), feqa mean {rep.fleet['feqa_mean']:.3f}")
        if tag == "LOAD":
            assert rep.fleet["n_overloaded"] == 0 and (rep.xf_day["peak_ratio"] <= 1.0).all() and len(rep.overloaded) == 0
        if tag.startswith("ind"):
            assert rep.fleet["n_overloaded"] > 0
    print("the distributed schedule ages the fleet", "less" if lol["dis_a90_r4800_P_res"] < lol["ind_a90_r4800_P_res"] else "more",
          "than the individual one")


def test_engine_transformer_report(gpu_lib):
    """After a short streaming run: transformer_report() of the schedule, of a rule schedule and of the base load against
    the restatement; the run's state keeps its bytes.  An engine built without feeder= reports the same bytes."""
    from test_gpu_losses import _small_workload
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.transformers import build_csr
    w = _small_workload()
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg")
    e = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, feeder=w.feeder, **kw)
    e.run(3)
    e.run_steps(10)
    before = [t.clone() for t in (e.P_est, e.P_sch, e.G)]
    xf_of = np.arange(w.M) // 4
    xf_of[5] = -1
    K = int(xf_of.max()) + 1
    kva = np.random.default_rng(2).choice([100.0, 167.0], K)
    xf_ptr, xf_rows = build_csr(xf_of, w.M, K)
    amb = np.full(24, 30.0)
    rep = e.transformer_report(xf_of, kva)
    assert rep.slot_hours == 1.0 and rep.load.shape == (K, 24)
    g = np.zeros((w.M, 24))
    np.add.at(g, w.node_of, w.load.astype(np.float64) + e.result()[0].astype(np.float64))
    check_report(rep, g, xf_ptr, xf_rows, kva * 0.95, amb, tag="engine")
    prof = e.rule_schedule("uncontrolled")
    rule = e.transformer_report(xf_of, kva, profile=prof, substeps=4, slot_hours=0.5, hot_limit=80.0, ambient=amb + 5.0)
    prof_h = (prof if isinstance(prof, np.ndarray) else prof.cpu().numpy()[e.inv_perm]).astype(np.float64)
    g2 = np.zeros((w.M, 24))
    np.add.at(g2, w.node_of, prof_h)
    check_report(rule, g2, xf_ptr, xf_rows, kva * 0.95, amb + 5.0, substeps=4, slot_hours=0.5, hot_limit=80.0, tag="rule")
    base = e.transformer_report(xf_of, kva, profile=w.load, arrays=False)
    assert base.load is None and base.fleet["energy_kwh"] > 0 and base.fleet["energy_kwh"] != rep.fleet["energy_kwh"]
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(before, (e.P_est, e.P_sch, e.G)))
    e.run_steps(2)
    dense = AdmmEngine(w.cost, w.homes, w.load, w.node_of, w.Rn, **kw)       # no feeder tree: the report needs none
    again = dense.transformer_report(xf_of, kva, profile=w.load, arrays=False)
    for k in RECORDS:
        assert getattr(again, k).tobytes() == getattr(base, k).tobytes(), k


def test_ensemble_transformer_reports_equal_single_engines(gpu_lib):
    """AdmmEnsemble.transformer_reports()[s] holds the bytes of a single engine's report on scenario s; the hot-spot
    tensor can stay on the device."""
    import torch
    from revs_admm_amd.engine import AdmmEngine
    from revs_admm_amd.ensemble import AdmmEnsemble
    from test_gpu_bound_many import _engine_case
    w, homes, load, _, _ = _engine_case(3)
    kw = dict(kappa=w.kappa, vset=w.vset, vlow=w.vlow, vhigh=w.vhigh, mode="pdhg", feeder=w.feeder)
    ens = AdmmEnsemble(w.cost, homes, load, w.node_of, w.Rn, **kw)
    ens.run(3)
    before = ens.P_sch.clone()
    xf_of = np.arange(w.M) % 7
    kva = np.full(7, 400.0)
    out = torch.zeros(3, 7, 24, dtype=torch.float64, device=ens.dev)
    reps = ens.transformer_reports(xf_of, kva, substeps=2, out=out)
    assert ens.P_sch.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for s in range(3):
        e = AdmmEngine(w.cost, homes[s], load[s], w.node_of, w.Rn, **kw)
        e.set_state(*ens.get_state(s))
        one = e.transformer_report(xf_of, kva, profile=e.P_sch, substeps=2)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(reps[s], k).tobytes(), (s, k)
        assert out[s].cpu().numpy().tobytes() == one.hot_spot.tobytes()
        assert one.fleet["n_nan"] == 0 and one.fleet["energy_kwh"] > 0


SHARD_CASE = dict(name="xf", mode="pdhg", n=20000, nodes=512, seed=0, stress=1.0, T=24, steps=4)


def test_sharded_report_is_bit_identical(gpu_lib, tmp_path):
    """Residences sharded node-aligned over two processes (gloo), a fresh child process per rank: both ranks' reports of
    the whole fleet -- of the schedule after 4 iterations and of a given profile -- hold the one-rank bytes."""
    sys.path.insert(0, HERE)
    from network_worker import engine
    from sharded_worker import make_case
    from transformers_worker import reports
    w = make_case(SHARD_CASE)
    ref = reports(engine(w, 0, len(w.load), None, None), w, 0, len(w.load), SHARD_CASE["steps"])
    assert np.isfinite(ref["sch_hot_spot"]).all()
    port = 29900 + (os.getpid() + 1543) % 2000
    procs = []
    for r in range(2):
        path = tmp_path / f"spec{r}.json"
        path.write_text(json.dumps(dict(rank=r, world=2, port=port, outdir=str(tmp_path), case=SHARD_CASE)))
        env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2", MKL_NUM_THREADS="2")
        log = open(tmp_path / f"w{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "transformers_worker.py"), str(path)], stdout=log,
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
        got = np.load(tmp_path / f"xf_r{r}.npz")
        assert sorted(got.files) == sorted(ref)
        for k in ref:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (r, k)


@pytest.mark.parametrize("path", ["upload", "device"])
def test_study_fills_transformers(gpu_lib, golden, path):
    """REVS.study(transformers=...) on the 121144 feeder, on the upload path (a dict of options) and on the ensemble's
    device path (True: owners from the labels, ratings from the base load): StudyReport.transformers[s] holds the bytes
    of report_for_rows on the report's own row s; the default leaves it None."""
    from test_gpu_losses import _study_inputs
    from revs_admm_amd.revs_fixture import REVS
    from revs_admm_amd.transformers import report_for_rows, rows_by_transformer, size_ratings
    tariff, all_homes, dist, com, _feeder = _study_inputs(golden)
    res = [n for n in dist if dist.nodes[n]["label"] == "H"]
    xf_of = rows_by_transformer(dist, res)[1]
    base = np.zeros((462, 24))
    np.add.at(base, xf_of, np.array([all_homes[h] for h in res], np.float64))
    kva = size_ratings(base.max(axis=1), pf=0.95)
    if path == "upload":
        grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234, 56), methods=("individual", "uncontrolled"), arrays=True)
        assert REVS().study(tariff, all_homes, dist, com, **dict(grid, seeds=(1234,), methods=("uncontrolled",)))[1].transformers is None
        opts = dict(substeps=2, hot_limit=100.0, ambient=25.0)
    else:
        grid = dict(adoptions=(90,), ratings=(4800,), seeds=(1234,), methods=("distributed", "individual"), arrays=True,
                    ensemble=True, device_report=True, max_iterations=2, v0=1.03, mode="relaxed")
        opts = {}
    labels, rep = REVS().study(tariff, all_homes, dist, com, transformers=opts or True, **grid)
    assert len(rep.transformers) == len(labels) == (4 if path == "upload" else 2)
    for s, got in enumerate(rep.transformers):
        one = report_for_rows(rep.node_p[s], xf_of, kva, **opts)
        for k in ARRAYS + RECORDS:
            assert getattr(one, k).tobytes() == getattr(got, k).tobytes(), (s, k)
        assert got.fleet["n_nan"] == 0 and got.fleet["n_xf"] == 462 and got.slot_hours == 1.0
