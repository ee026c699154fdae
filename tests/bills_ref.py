"""numpy yard-stick of the bill report (test-centralopt.py:112-116): the sequential bill loop, the deviation formula as
numpy evaluates it, numpy.percentile / boxplot_stats records (network_ref.box_stats) and math.fsum for the total.
Nothing here knows how the device maps rows to threads, selects or sums."""
import math

import numpy as np

import network_ref as nr


def bills(g, tariff):
    """g (..., T) of any float type, tariff (T,) float64 -> (...) float64: one accumulator from +0.0, the slots
    ascending, product and sum rounded separately."""
    g = np.asarray(g)
    c = np.asarray(tariff, np.float64)
    acc = np.zeros(g.shape[:-1], np.float64)
    for t in range(g.shape[-1]):
        acc = acc + c[t] * g[..., t].astype(np.float64)
    return acc


def deviations(bill, base):
    """bill (S, n), base (S,) -> dev (S, n) = 100 (C2 - C1) / C1 against row base[s]; a row of NaN where base[s] < 0."""
    dev = np.full(bill.shape, np.nan)
    with np.errstate(all="ignore"):
        for s, b in enumerate(base):
            if b >= 0:
                dev[s] = 100 * (bill[s] - bill[b]) / bill[b]
    return dev


def record(values, keep, members, index_of_row=None):
    """The record over values[s][i] for s in members (ascending), keep[s][i] true: dict.  values (S, n); keep (S, n)
    bool or None; index_of_row (n,) or None.  worst: the largest value, the lowest scenario, then the lowest caller-side
    index on ties."""
    n = values.shape[1]
    ior = np.arange(n) if index_of_row is None else np.asarray(index_of_row)
    xs, ss, ii, n_nan = [], [], [], 0
    for s in members:
        k = np.ones(n, bool) if keep is None else np.asarray(keep[s], bool)
        v = values[s][k] + 0.0
        fin = np.isfinite(v)
        n_nan += int((~fin).sum())
        xs.append(v[fin]); ss.append(np.full(int(fin.sum()), s)); ii.append(ior[k][fin])
    x = np.concatenate(xs) if xs else np.zeros(0)
    rec = dict(count=int(x.size), n_nan=n_nan, n_above=int((x > 0.0).sum()), worst_index=-1, worst_scenario=-1,
               box=nr.box_stats(x), total=math.fsum(x) if x.size else np.nan, abs_total=math.fsum(np.abs(x)))
    if x.size:
        ss, ii = np.concatenate(ss), np.concatenate(ii)
        top = np.flatnonzero(x == x.max())
        j = top[np.lexsort((ii[top], ss[top]))[0]]
        rec["worst_scenario"], rec["worst_index"] = int(ss[j]), int(ii[j])
    return rec


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_record(got, ref, what=""):
    """A BILL_DTYPE record against record(): counts, extremes, whiskers and the worst entry exactly, the quartiles within
    2 ulps, the total within count 2^-53 sum|x| of math.fsum (the worst case of any summation order)."""
    ints = ("count", "n_nan", "n_above", "worst_index", "worst_scenario")
    assert tuple(int(got[k]) for k in ints) == tuple(ref[k] for k in ints), (what, got, ref)
    assert got["reserved0"] == 0.0
    if ref["count"] == 0:
        assert int(got["n_fliers"]) == 0, (what, got)
        for k in ("min", "q1", "median", "q3", "max", "whisker_lo", "whisker_hi", "total"):
            assert np.isnan(got[k]), (what, k, got)
        return
    b = ref["box"]
    assert int(got["n_fliers"]) == b["n_fliers"], (what, got, b)
    for k in ("min", "max", "whisker_lo", "whisker_hi"):
        assert got[k] == b[k] and not (got[k] == 0.0 and np.signbit(got[k])), (what, k, got[k], b[k])
    for k in ("q1", "median", "q3"):
        assert got[k] == b[k] or ulps(got[k], b[k]) <= 2, (what, k, got[k], b[k])
    assert abs(got["total"] - ref["total"]) <= ref["count"] * 2.0 ** -53 * ref["abs_total"], (what, got["total"], ref)


def check_report(rep, bill, dev, keep, index_of_row=None, what=""):
    """Every record of a BillReport-like (summary_bill / summary_dev / pooled_bill / pooled_dev, groups) against the
    yard-stick on the arrays given."""
    S = bill.shape[0]
    for q, (name, vals) in enumerate((("bill", bill), ("dev", dev))):
        for s in range(S):
            check_record(getattr(rep, "summary_" + name)[s], record(vals, keep, [s], index_of_row), (what, name, "scenario", s))
        for g in range(rep.n_groups):
            members = np.flatnonzero(np.asarray(rep.groups) == g)
            check_record(getattr(rep, "pooled_" + name)[g], record(vals, keep, members, index_of_row), (what, name, "group", g))


def same_report(a, b):
    """Two BillReports agree in every byte."""
    for k in ("bill", "dev", "keep"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        assert x is None or (x.shape == y.shape and x.tobytes() == y.tobytes()), k
    for k in ("summary_bill", "summary_dev", "pooled_bill", "pooled_dev"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert a.base.tolist() == b.base.tolist() and a.groups.tolist() == b.groups.tolist() and a.n_groups == b.n_groups
