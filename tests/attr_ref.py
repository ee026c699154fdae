"""float64 numpy restatement of the attribution report (include/revs_admm_ops.h, "attribution report"): the contract.

  sens_row()   wc[lca(i, j*)] by a parent walk: j*'s root path is marked by stepping to the parent, then every position
               takes its own wc when marked, else what its parent took (parents come first in preorder).  Nothing in it
               knows about prefix or suffix maxima.
  contract()   from given drops (the kernel's own drop_out, or tree_report_host's): the watch rule, the products, the
               fixed binary tree of the sums (losses_ref.tree_sum), the counts, the top 8, the box-plot record
               (network_ref.box_stats) and the day loops.

Everything is indexed by preorder position, as feeder_tree lays the nodes out; headroom_ref.to_pos / to_nodes convert."""
import numpy as np

import network_ref as nr
from headroom_ref import to_nodes, to_pos  # noqa: F401  (re-exported)
from losses_ref import tree_sum


def sens_row(aux, jstar):
    """sens (n,) by position for the watched position jstar (-1: all +0.0)."""
    parent, wc = np.asarray(aux["parent_pos"], np.int64), np.asarray(aux["wc"], np.float64)
    n = len(parent)
    marked = np.zeros(n, bool)
    j = int(jstar)
    while j >= 0:
        marked[j] = True
        j = int(parent[j])
    s = np.zeros(n)
    for i in range(n):
        if marked[i]:
            s[i] = wc[i]
        elif parent[i] >= 0:
            s[i] = s[parent[i]]
    return s


def pick_watch(order, lim, drop_t):
    """The limit position of largest drop, ties to the lowest caller-side index; -1 without a candidate."""
    cand = np.flatnonzero(lim)
    if not cand.size:
        return -1
    at = cand[drop_t[cand] == drop_t[cand].max()]
    return int(at[np.argmin(order[at])])


def contract(tree, aux, n_nodes, inj, ev, drop, drop_max, frac, limit=None, out_mask=None, cls=None, C=0, watch_pos=-1,
             bad=None):
    """inj, ev (or None), drop: (n, T) by position.  limit / out_mask: (n,) bool by position or None (the positions with a
    row / all); cls: (n,) integers by position or None; bad: (T,) bool or None (derived from inj and ev).
    -> dict(sens, contrib, ev_contrib (n, T) by position; slot: dict of (T, ...) arrays; summary: list of T dicts;
    day: dict of (n_nodes,) arrays in the caller's order)."""
    n, T = drop.shape
    order = np.asarray(tree["order"], np.int64)
    has = order < n_nodes
    evv = np.zeros((n, T)) if ev is None else np.asarray(ev, np.float64)
    lim = has & ((np.asarray(tree["src"]) >= 0) if limit is None else np.asarray(limit, bool))
    om = has & (np.ones(n, bool) if out_mask is None else np.asarray(out_mask, bool))
    if bad is None:
        bad = ~(np.isfinite(inj).all(axis=0) & np.isfinite(evv).all(axis=0))
    sens, con, evc = np.zeros((n, T)), np.zeros((n, T)), np.zeros((n, T))
    reach, isbig = np.zeros((n, T), bool), np.zeros((n, T), bool)
    f8, i4 = lambda *s: np.zeros(s), lambda *s: np.zeros(s, np.int32)
    slot = dict(drop_watch=f8(T), excess=f8(T), total=f8(T), ev_total=f8(T), class_total=f8(T, 4),
                top_value=np.full((T, 8), np.nan), top_index=np.full((T, 8), -1, np.int32), watch=np.full(T, -1, np.int32),
                n_reach=i4(T), n_big=i4(T), n_can=i4(T), n_bad=bad.astype(np.int32))
    none = np.zeros(T, bool)
    for t in range(T):
        if bad[t]:
            sens[:, t], con[:, t], evc[:, t] = np.nan, np.nan, np.nan
            for k in ("drop_watch", "excess", "total", "ev_total", "class_total"):
                slot[k][t] = np.nan
            continue
        j = int(watch_pos) if watch_pos >= 0 else pick_watch(order, lim, drop[:, t])
        if j < 0:
            none[t] = True
            continue
        s = sens_row(aux, j)
        with np.errstate(over="ignore", invalid="ignore"):
            c, e = s * inj[:, t], s * evv[:, t]
        sens[:, t], con[:, t], evc[:, t] = s, c, e
        dw = drop[j, t]
        over = dw - drop_max
        excess = over if over > 0.0 else 0.0
        slot["drop_watch"][t], slot["excess"][t] = dw, excess
        slot["watch"][t] = order[j] if has[j] else -1
        slot["total"][t], slot["ev_total"][t] = tree_sum(c), tree_sum(e)
        for k in range(C):
            slot["class_total"][t, k] = tree_sum(np.where(np.asarray(cls) == k, c, 0.0))
        r = om & (s > 0.0)
        big = r & (c > frac * dw)
        with np.errstate(divide="ignore", invalid="ignore"):
            can = r & (excess > 0.0) & (excess / np.where(s > 0.0, s, 1.0) <= evv[:, t])
        reach[:, t], isbig[:, t] = r, big
        slot["n_reach"][t], slot["n_big"][t], slot["n_can"][t] = r.sum(), big.sum(), can.sum()
        top = sorted((-c[p], int(order[p])) for p in np.flatnonzero(r) if not np.isnan(c[p]))[:8]
        for k, (v, i) in enumerate(top):
            slot["top_value"][t, k], slot["top_index"][t, k] = -v, i
    # ---- the box-plot record of the contributions of the nodes that reach the watched one
    summary = []
    for t in range(T):
        if bad[t] or none[t]:
            summary.append(dict(n_nan=int(om.sum()) if bad[t] else 0, count=0, n_violations=0, worst_index=-1,
                                worst_value=np.nan, n_zero=0, box=None))
            continue
        pos = np.flatnonzero(reach[:, t] & ~np.isnan(con[:, t]))
        x, xi = con[pos, t], order[pos]
        rec = dict(n_nan=int((om & np.isnan(con[:, t])).sum()), count=int(x.size), n_violations=int(isbig[:, t].sum()),
                   worst_index=-1, worst_value=np.nan, n_zero=int((om & ~reach[:, t] & ~np.isnan(con[:, t])).sum()),
                   box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.max())
            rec["worst_index"] = int(xi[x == x.max()].min())
        summary.append(rec)
    # ---- the day of every node: by position, then in the caller's order
    dsum, desum, peak = np.zeros(n), np.zeros(n), np.full(n, np.nan)
    pslot, nbig = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for j in range(n):
        for t in range(T):
            if bad[t]:
                continue
            v = con[j, t]
            if slot["excess"][t] > 0.0:
                dsum[j] = dsum[j] + v
                if ev is not None:
                    desum[j] = desum[j] + evc[j, t]
            if pslot[j] < 0 or v > peak[j]:
                peak[j], pslot[j] = v, t
            nbig[j] += isbig[j, t]
    day = {}
    for k, a in (("sum", dsum), ("ev_sum", desum), ("peak", peak), ("peak_slot", pslot), ("n_big", nbig)):
        out = np.zeros(n_nodes, a.dtype)
        out[order[has]] = a[has]
        day[k] = out
    return dict(sens=sens, contrib=con, ev_contrib=evc, slot=slot, summary=summary, day=day, reach=reach, bad=bad)


def relief(sens, excess):
    """excess / sens where sens > 0, +inf where sens = 0 and excess > 0, 0 where excess = 0 (sens (n, T), excess (T,))."""
    ex = np.asarray(excess, np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(sens > 0.0, ex / np.where(sens > 0.0, sens, 1.0), np.inf)
    return np.where(ex == 0.0, 0.0, r)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_summary(got, want):
    """A device summary record array (T,) against contract()'s list: == for the order statistics and the counts, <= 2 ulp
    for the interpolated quartiles (test_gpu_network.check_summary's rule)."""
    for t, r in enumerate(want):
        g = got[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"], g["reserved"][0]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"], r["n_zero"]), (t, g, r)
        if r["count"] == 0:
            assert np.isnan(g["min"]) and np.isnan(g["median"]) and np.isnan(g["worst_value"]) and g["n_fliers"] == 0
            continue
        b = r["box"]
        for k in ("min", "max", "whisker_lo", "whisker_hi"):
            assert g[k] == b[k], (t, k, g[k], b[k])
        assert g["worst_value"] == r["worst_value"]
        for k in ("q1", "median", "q3"):
            assert ulps(g[k], b[k]) <= 2, (t, k, g[k], b[k])
        assert g["n_fliers"] == b["n_fliers"], (t, g, b)
