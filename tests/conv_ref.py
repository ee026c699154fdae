"""numpy yard-stick of the convergence report (lpsolver.py:280-290, diff[h][k]; test-dist-ind-opt.py:109-120,
plot_convergence): numpy.percentile / boxplot_stats records (network_ref.box_stats), math.fsum for the totals, and the
per-residence and per-scenario definitions as plain loops over the rows.  Nothing here knows how the device maps columns
to threads, selects or sums.  Histories are (S, K, n): scenario, row, residence (row i of the device's history)."""
import math

import numpy as np

import bills_ref as br
import network_ref as nr


def record(values, keep, members, eps, index_of_row=None):
    """bills_ref.record over values (S, n) -- the kept, finite values of the members -- with n_above the values > eps."""
    rec = br.record(np.asarray(values, np.float64), keep, members, index_of_row)
    n = values.shape[1]
    above = 0
    for s in members:
        k = np.ones(n, bool) if keep is None else np.asarray(keep[s], bool)
        v = np.asarray(values[s], np.float64)[k]
        above += int((v[np.isfinite(v)] > eps).sum())
    rec["n_above"] = above
    return rec


def iteration_records(hist, eps, keep=None, index=None):
    """-> [S][K] dicts: scenario s's kept residuals at row k."""
    S, K, n = hist.shape
    return [[record(hist[:, k, :], keep, [s], eps, index) for k in range(K)] for s in range(S)]


def pooled_records(hist, eps, groups, G, keep=None, index=None):
    S, K, n = hist.shape
    out = []
    for g in range(G):
        members = [s for s in range(S) if groups[s] == g]
        out.append([record(hist[:, k, :], keep, members, eps, index) for k in range(K)])
    return out


def residence(col, eps):
    """One residence's column of K float32 residuals -> dict(max, last, settle, n_above, worst_iteration)."""
    n_above, last_above, mx, wi = 0, -1, None, -1
    for k, x in enumerate(col):
        x = np.float32(x)
        if not (float(x) <= eps):
            n_above += 1
            last_above = k
        if not np.isnan(x) and (mx is None or x > mx):
            mx, wi = x, k
    return dict(max=np.float32(np.nan) if mx is None else np.float32(mx + np.float32(0.0)), last=np.float32(col[-1]),
                settle=last_above + 1, n_above=n_above, worst_iteration=wi)


def run_record(maxima, eps, patience, settles=None):
    """maxima: the K values m[k] of a scenario's iteration records (NaN: an empty sample); settles: the kept residences'
    settle values, or None (the counts are then -1)."""
    K = len(maxima)
    within = [bool(m <= eps) for m in maxima]
    converged_at = -1
    for k0 in range(K):
        if k0 + patience <= K and all(within[k0:k0 + patience]):
            converged_at = k0
            break
    last_above = max([k for k in range(K) if not within[k]], default=-1)
    if settles is None:
        return dict(converged_at=converged_at, last_above=last_above, n_unsettled=-1, n_never=-1)
    return dict(converged_at=converged_at, last_above=last_above, n_unsettled=sum(1 for v in settles if v == K),
                n_never=sum(1 for v in settles if v == 0))


def settle_record(settles, index):
    """The record over the kept residences' settle (a list of small integers) and their caller-side indices."""
    x = np.asarray(settles, np.float64)
    rec = dict(count=int(x.size), n_nan=0, n_above=int((x > 0).sum()), worst_index=-1, worst_scenario=-1,
               box=nr.box_stats(x), total=math.fsum(x) if x.size else np.nan)
    if x.size:
        top = np.flatnonzero(x == x.max())
        rec["worst_index"] = int(min(np.asarray(index)[top]))
    return rec


def check_record(got, ref, what=""):
    """bills_ref.check_record: counts, extremes, whiskers, worst entries and all integer fields exactly, quartiles equal
    or within 2 ulps, total within count 2^-53 sum|x| of math.fsum."""
    br.check_record(got, ref, what)


def check_settle_record(got, ref, s, what=""):
    """Exact in every field."""
    assert int(got["count"]) == ref["count"] and int(got["n_nan"]) == 0 and got["reserved0"] == 0.0, (what, got, ref)
    if ref["count"] == 0:
        assert int(got["n_fliers"]) == 0 and int(got["n_above"]) == 0, (what, got)
        assert int(got["worst_index"]) == -1 and int(got["worst_scenario"]) == -1, (what, got)
        for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi", "total"):
            assert np.isnan(got[k]), (what, k, got)
        return
    b = ref["box"]
    assert int(got["n_above"]) == ref["n_above"] and int(got["n_fliers"]) == b["n_fliers"], (what, got, ref)
    assert int(got["worst_index"]) == ref["worst_index"] and int(got["worst_scenario"]) == s, (what, got, ref)
    for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi"):
        assert got[k] == b[k], (what, k, got[k], b[k])
    assert got["total"] == ref["total"], (what, got["total"], ref["total"])


def check_report(rep, hist, eps, patience, keep=None, index=None, groups=None, what=""):
    """Every record of a ConvergenceReport-like (iterations, pooled, settle, run, residences -- the last in the
    history's row order, or None) against the yard-stick on hist (S, K, n) float32."""
    hist = np.asarray(hist, np.float32)
    S, K, n = hist.shape
    idx = np.arange(n) if index is None else np.asarray(index)
    it = iteration_records(hist, eps, keep, index)
    for s in range(S):
        for k in range(K):
            check_record(rep.iterations[s, k], it[s][k], (what, "scenario", s, "row", k))
            if it[s][k]["count"]:
                assert int(rep.iterations[s, k]["worst_scenario"]) == s
    if groups is not None:
        G = int(max(groups)) + 1
        assert rep.pooled.shape == (G, K)
        pr = pooled_records(hist, eps, groups, G, keep, index)
        for g in range(G):
            for k in range(K):
                check_record(rep.pooled[g, k], pr[g][k], (what, "group", g, "row", k))
    res = [[residence(hist[s, :, i], eps) for i in range(n)] for s in range(S)]
    if rep.residences is not None:
        assert rep.residences.shape == (S, n)
        for s in range(S):
            for i in range(n):
                got, ref = rep.residences[s, i], res[s][i]
                for k in ("settle", "n_above", "worst_iteration"):
                    assert int(got[k]) == ref[k], (what, s, i, k, got, ref)
                assert int(got["reserved"]) == 0
                for k in ("max", "last"):
                    assert got[k].tobytes() == ref[k].tobytes() or (np.isnan(got[k]) and np.isnan(ref[k])), \
                        (what, s, i, k, got, ref)
    for s in range(S):
        kept = [i for i in range(n) if keep is None or keep[s][i]]
        settles = [res[s][i]["settle"] for i in kept]
        if rep.settle is not None:
            check_settle_record(rep.settle[s], settle_record(settles, idx[kept]), s, (what, "settle", s))
        if rep.run is not None:
            maxima = [it[s][k]["box"]["max"] if it[s][k]["count"] else np.nan for k in range(K)]
            want = run_record(maxima, eps, patience, settles if rep.residences is not None else None)
            got = {k: int(rep.run[s][k]) for k in want}
            assert got == want, (what, "run", s, got, want)
