"""numpy yard-stick of the statistics across scenarios (revs_net_across, study.AcrossReport).  Per cell: the members'
values in ascending scenario order, NaNs dropped, numpy.percentile for the five order statistics, the mean by an
explicit float64 loop, counts by numpy's comparisons, the worst scenario by argmax (the first occurrence: the lowest
scenario).  Nothing here knows how the device selects.  Cells whose members are all numbers go through ONE
numpy.percentile call along the member axis -- the same function, the same rule, cell by cell the same arithmetic;
cells with a NaN are taken one by one."""
import numpy as np

from revs_admm_amd._lib import ACROSS_DTYPE

QS = ("min", "q1", "median", "q3", "max")


def empty(shape):
    out = np.zeros(shape, ACROSS_DTYPE)
    for k in QS + ("mean",):
        out[k] = np.nan
    out["worst_scenario"] = -1
    return out


def cell(v, lo, hi, sense, bands, scen=None):
    """One cell: v the members' values in ascending scenario order, scen their scenario indices -> a record."""
    v = np.asarray(v, np.float64)
    scen = np.arange(len(v)) if scen is None else np.asarray(scen)
    r = empty(())
    ok = ~np.isnan(v)
    r["n_nan"] = int((~ok).sum())
    v, scen = v[ok], scen[ok]
    r["count"] = len(v)
    if len(v) == 0:
        return r
    q = np.percentile(v, [0, 25, 50, 75, 100])
    for k, x in zip(QS, q):
        r[k] = x
    acc = np.float64(0.0)
    for x in v:
        acc = acc + x
    r["mean"] = acc / np.float64(len(v))
    r["n_violations"] = int(((v < lo) | (v > hi)).sum())
    r["worst_scenario"] = int(scen[np.argmax(np.fmax(lo - v, v - hi))])
    for b, th in enumerate(bands):
        r["band_count"][b] = int((v <= th).sum() if sense < 0 else (v >= th).sum())
    return r


def across_cells(values, keep, groups, n_groups, lo, hi, sense, bands):
    """values (S, n, T) -> (G, n, T) records; keep (n,) bool or None."""
    values = np.asarray(values, np.float64)
    S, n, T = values.shape
    groups = np.asarray(groups)
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    out = empty((n_groups, n, T))
    with np.errstate(invalid="ignore"):
        for g in range(n_groups):
            mem = np.flatnonzero(groups == g)
            if len(mem) == 0:
                continue
            V = values[mem][:, keep]                             # (k, kept, T)
            ok = ~np.isnan(V)
            rec = empty(V.shape[1:])
            rec["count"] = ok.sum(0)
            rec["n_nan"] = (~ok).sum(0)
            whole = ok.all(0)
            if whole.any():
                q = np.percentile(V[:, whole], [0, 25, 50, 75, 100], axis=0)
                for k, x in zip(QS, q):
                    rec[k][whole] = x
                acc = np.zeros(int(whole.sum()))
                for j in range(len(mem)):                        # (ascending scenario order, from +0.0)
                    acc = acc + V[j][whole]
                rec["mean"][whole] = acc / np.float64(len(mem))
                Vw = V[:, whole]
                rec["n_violations"][whole] = ((Vw < lo) | (Vw > hi)).sum(0)
                rec["worst_scenario"][whole] = mem[np.argmax(np.fmax(lo - Vw, Vw - hi), axis=0)]
                bc = rec["band_count"]
                for b, th in enumerate(bands):
                    bc[whole, b] = (Vw <= th).sum(0) if sense < 0 else (Vw >= th).sum(0)
            for i, t in zip(*np.nonzero(~whole)):
                rec[i, t] = cell(V[:, i, t], lo, hi, sense, bands, mem)
            out[g][keep] = rec
    return out


def daily_extreme(values, sense):
    values = np.asarray(values, np.float64)
    return values.min(axis=2) if sense < 0 else values.max(axis=2)


def exposure(values, keep, groups, n_groups, lo, hi):
    values = np.asarray(values, np.float64)
    S, n, T = values.shape
    groups = np.asarray(groups)
    out = np.zeros((n_groups, n), np.int32)
    with np.errstate(invalid="ignore"):
        bad = ((values < lo) | (values > hi)).sum(axis=2)
    for g in range(n_groups):
        out[g] = bad[groups == g].sum(axis=0)
    if keep is not None:
        out[:, ~np.asarray(keep, bool)] = 0
    return out


def across(values, keep, groups, n_groups, lo, hi, sense, bands, slots=True):
    """-> (slot (G, n, T) or None, daily (G, n), exposure (G, n)): revs_net_across's three outputs."""
    slot = across_cells(values, keep, groups, n_groups, lo, hi, sense, bands) if slots else None
    daily = across_cells(daily_extreme(values, sense)[:, :, None], keep, groups, n_groups, lo, hi, sense, bands)[:, :, 0]
    return slot, daily, exposure(values, keep, groups, n_groups, lo, hi)


CALLS = []


def host_across(lib, stream, values, keep, groups, n_groups, lo, hi, sense, bands, slots):
    """study.native_across's stand-in on the host: the yard-stick on the values it is handed (a torch tensor)."""
    CALLS.append(dict(shape=tuple(values.shape), keep=None if keep is None else np.asarray(keep).copy(),
                      groups=np.asarray(groups).tolist(), n_groups=n_groups, lo=lo, hi=hi, sense=sense, bands=tuple(bands),
                      slots=slots))
    return across(values.cpu().numpy(), keep, groups, n_groups, lo, hi, sense, bands, slots)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def same_numbers(a, b):
    """a == b where both are numbers, and NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and (a[~np.isnan(a)] == b[~np.isnan(b)]).all())


def check_records(got, ref, what=""):
    """Records of the device against the yard-stick's: the integers, min, max and mean exactly, the quartiles within
    2 ulps (the bar study_ref.check_pooled holds the same np_lerp to)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for k in ("count", "n_nan", "n_violations", "worst_scenario", "band_count"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5])
    for k in ("min", "max", "mean"):
        assert same_numbers(got[k], ref[k]), (what, k)
    for k in ("q1", "median", "q3"):
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), (what, k)
        same = got[k] == ref[k]                                   # (equal infinities are 0 ulps apart)
        with np.errstate(invalid="ignore"):
            far = ~nan & ~same & ~(ulps(got[k], ref[k]) <= 2)
        assert not far.any(), (what, k, got[k][far][:5], ref[k][far][:5])


def host_study(parent, edge_r, cons_of, node_p, groups, n_groups, bands, rating, nodes, vset, vmin, vmax, arrays,
               device=None, across=False):
    """study.native_study's stand-in with its trailing across: tests/study_ref.host_study for the report, and -- as
    native_study_device does with the arrays on the device -- study.across_report_device on its arrays."""
    import torch
    import study_ref as sr
    from revs_admm_amd import study
    rep = sr.host_study(parent, edge_r, cons_of, node_p, groups, n_groups, bands, rating, nodes, vset, vmin, vmax, True)
    if across:
        rep.across = study.across_report_device(torch.from_numpy(rep.volt),
                                                None if rating is None else torch.from_numpy(rep.loading), groups,
                                                nodes=nodes, rated=rating, bands=bands, vmin=vmin, vmax=vmax)
    if not arrays:
        rep.flow = rep.loading = rep.volt = None
    return rep


def host_study_device(feeder, seen=None):
    """-> study.native_study_device's stand-in on `feeder` = (parent, edge_r, cons_of)."""
    def native_study_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, groups, n_groups, bands, rating, nodes,
                            vset, vmin, vmax, arrays, across=False):
        if seen is not None:
            seen.append(dict(arrays=arrays, across=across, n_groups=n_groups))
        return host_study(*feeder, node_g.numpy().copy(), groups, n_groups, bands, rating, nodes, vset, vmin, vmax, arrays,
                          across=across)
    return native_study_device


def check_report(acr, volt, loading, groups, nodes, rating, bands, loading_bands, vmin, vmax, slots=True):
    """An AcrossReport against the yard-stick on the arrays it was made from (volt, loading: (S, n, T) numpy)."""
    groups = np.asarray(groups)
    G, n = int(groups.max()) + 1, volt.shape[1]
    keep_v = None
    if nodes is not None:
        keep_v = np.zeros(n, bool)
        keep_v[np.asarray(nodes)] = True
    todo = [("volt", volt, keep_v, vmin, vmax, -1, bands)]
    if loading is not None:
        keep_l = None if rating is None else np.nan_to_num(np.asarray(rating, np.float64)) > 0
        todo.append(("loading", loading, keep_l, -np.inf, 1.0, 1, loading_bands))
    else:
        assert acr.slot_loading is None and acr.daily_loading is None and acr.exposure_loading is None
    for kind, values, keep, lo, hi, sense, bd in todo:
        slot, daily, expo = across(values, keep, groups, G, lo, hi, sense, bd, slots)
        if slots:
            check_records(getattr(acr, "slot_" + kind), slot, "slot_" + kind)
        else:
            assert getattr(acr, "slot_" + kind) is None
        check_records(getattr(acr, "daily_" + kind), daily, "daily_" + kind)
        assert np.array_equal(getattr(acr, "exposure_" + kind), expo), kind
    assert acr.group_sizes.tolist() == [int((groups == g).sum()) for g in range(G)]
    assert acr.bands_volt == tuple(bands) and acr.bands_loading == tuple(loading_bands)


def same_across(a, b):
    """Two AcrossReports, bit for bit."""
    for k in ("slot_volt", "slot_loading", "daily_volt", "daily_loading", "exposure_volt", "exposure_loading",
              "group_sizes"):
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None) or (x is not None and x.tobytes() != y.tobytes()):
            return False
    return a.bands_volt == b.bands_volt and a.bands_loading == b.bands_loading
