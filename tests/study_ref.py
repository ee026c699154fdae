"""numpy yard-stick of the study report: network_ref.summary applied to the concatenation of a group's arrays, and the
band counts by numpy's own `<=`.  Nothing here knows how the device pools or counts."""
import numpy as np

import network_ref as nr


def band_counts(volt, nodes, bands):
    """volt (S, n, T) -> (S, T, B) int: nodes of `nodes` (None: all) with volt <= band (NaN: never)."""
    v = volt if nodes is None else volt[:, np.asarray(nodes)]
    with np.errstate(invalid="ignore"):
        return np.stack([(v <= b).sum(axis=1) for b in bands], axis=-1).astype(np.int32)


def pooled(values, keep, members, kind, vmin=None, vmax=None):
    """network_ref.summary over the values of scenarios `members` (ascending) stacked: values (S, n, T), keep (n,) bool.
    The worst entry's stacked index is split into (worst_scenario, worst_index): the lowest stacked index on ties is
    the lowest scenario, then the lowest index."""
    n = values.shape[1]
    if len(members) == 0:
        return [dict(n_nan=0, count=0, n_violations=0, worst_index=-1, worst_scenario=-1, worst_value=np.nan, box=None)
                for _ in range(values.shape[2])]
    recs = nr.summary(np.concatenate([values[s] for s in members], axis=0), np.tile(keep, len(members)), kind, vmin, vmax)
    for r in recs:
        j = r["worst_index"]
        r["worst_scenario"], r["worst_index"] = (int(members[j // n]), j % n) if j >= 0 else (-1, -1)
    return recs


def keep_masks(n, rating, nodes):
    rated = np.zeros(n, bool) if rating is None else (np.isfinite(rating) & (np.asarray(rating) > 0))
    keep = np.ones(n, bool)
    if nodes is not None:
        keep[:] = False
        keep[np.asarray(nodes)] = True
    return rated, keep


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_pooled(rep, rating, nodes):
    """rep's pooled records against the yard-stick on rep's OWN arrays: counts, extremes, whiskers and the worst entry
    exactly, the quartiles within 2 ulps (the bar test_gpu_network.check_summary holds the single report to)."""
    n = rep.volt.shape[1]
    rated, keep = keep_masks(n, rating, nodes)
    for g in range(rep.n_groups):
        members = np.flatnonzero(rep.groups == g)
        for rec, ref in ((rep.pooled_loading[g], pooled(rep.loading, rated, members, "loading")),
                         (rep.pooled_volt[g], pooled(rep.volt, keep, members, "volt", rep.vmin, rep.vmax))):
            for t, r in enumerate(ref):
                got = rec[t]
                assert (got["count"], got["n_nan"], got["n_violations"], got["worst_index"], got["worst_scenario"]) == \
                    (r["count"], r["n_nan"], r["n_violations"], r["worst_index"], r["worst_scenario"]), (g, t, got, r)
                if r["count"] == 0:
                    assert np.isnan(got["min"]) and np.isnan(got["median"]) and np.isnan(got["worst_value"])
                    assert got["n_fliers"] == 0
                    continue
                b = r["box"]
                for k in ("min", "max", "whisker_lo", "whisker_hi"):
                    assert got[k] == b[k], (g, t, k, got[k], b[k])
                assert got["worst_value"] == r["worst_value"], (g, t, got, r)
                for k in ("q1", "median", "q3"):
                    assert ulps(got[k], b[k]) <= 2, (g, t, k, got[k], b[k])
                assert got["n_fliers"] == b["n_fliers"], (g, t, got, b)


def check_bands(rep, nodes):
    assert np.array_equal(rep.band_counts, band_counts(rep.volt, nodes, rep.bands))


SHARED = ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi", "worst_value", "count", "n_fliers",
          "n_violations", "n_nan", "worst_index")


def same_shared_fields(pool_rec, summary_rec):
    """Every field revs_net_pooled_t shares with revs_net_summary_t, bit for bit."""
    return all(pool_rec[k].tobytes() == summary_rec[k].tobytes() for k in SHARED)


def _records(dtype, recs):
    out = np.zeros(len(recs), dtype)
    for t, r in enumerate(recs):
        b = r["box"] or {}
        for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi"):
            out[k][t] = b.get(k, np.nan)
        out["worst_value"][t] = r["worst_value"]
        out["n_fliers"][t] = b.get("n_fliers", 0)
        for k in ("count", "n_violations", "n_nan", "worst_index"):
            out[k][t] = r[k]
        if "worst_scenario" in dtype.names:
            out["worst_scenario"][t] = r["worst_scenario"]
    return out


def host_study(parent, edge_r, cons_of, node_p, groups, n_groups, bands, rating, nodes, vset, vmin, vmax, arrays,
               device=None):
    """study.native_study's stand-in on the host: the arrays by the numpy tree restatement (feeder.tree_report_host),
    every record by the yard-stick above."""
    from revs_admm_amd.feeder import feeder_tree, tree_report_host
    from revs_admm_amd.network import SUMMARY_DTYPE
    from revs_admm_amd.study import POOLED_DTYPE, StudyReport
    S, M, T = node_p.shape
    n = len(parent)
    tr = feeder_tree(parent, edge_r, cons_of, np.ones(M, bool))
    rt = np.full(n, np.nan) if rating is None else np.where(np.asarray(rating) > 0, rating, np.nan)
    flow, loading, volt = (np.empty((S, n, T)) for _ in range(3))
    for s in range(S):
        flow[s], drop = tree_report_host(tr, node_p[s], n)
        loading[s] = np.abs(flow[s]) / rt[:, None]
        with np.errstate(invalid="ignore"):
            volt[s] = np.sqrt(vset * vset - drop)
    rated, keep = keep_masks(n, rating, nodes)
    sl = np.stack([_records(SUMMARY_DTYPE, nr.summary(loading[s], rated, "loading")) for s in range(S)])
    sv = np.stack([_records(SUMMARY_DTYPE, nr.summary(volt[s], keep, "volt", vmin, vmax)) for s in range(S)])
    groups = np.asarray(groups, np.int64)
    mem = [np.flatnonzero(groups == g) for g in range(n_groups)]
    pl = np.stack([_records(POOLED_DTYPE, pooled(loading, rated, m, "loading")) for m in mem]) if n_groups else np.zeros((0, T), POOLED_DTYPE)
    pv = np.stack([_records(POOLED_DTYPE, pooled(volt, keep, m, "volt", vmin, vmax)) for m in mem]) if n_groups else np.zeros((0, T), POOLED_DTYPE)
    bc = band_counts(volt, nodes, bands) if len(bands) else np.zeros((S, T, 0), np.int32)
    keepa = (flow, loading, volt) if arrays else (None, None, None)
    return StudyReport(sl, sv, pl, pv, bc, tuple(bands), groups, *keepa, node_p, float(vset), float(vmin), float(vmax))
