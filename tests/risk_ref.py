"""float64 numpy restatement of the risk report (include/revs_admm_ops.h, "risk report"), in two forms.

  definition()  the variance of every node's drop from the dense R (headroom_ref.lca_matrix):
                var = (R * R) @ s2 + sum_k (R @ beta_k) ** 2.  Nothing in it knows about subtrees or w2.
  path_form()   the same variance the way the kernel takes it: the flow scan of s2, the drop scan with
                feeder.risk_weights' w2 in place of w, the clamp, and the drop scan of every loading -- in
                feeder.tree_report_host's order of additions, which is not the kernel's: the kernel's sd is held to its
                sqrt within BOUND x max(var) on var (test_gpu_network.BOUND, the project's figure for one order of a scan
                against another).
  contract()    everything behind var_ind, c_k and drop, FED THE KERNEL'S OWN drop and sd (attr_ref.contract's pattern:
                there the kernel's own drop): z, drop_q, the counts, z_min and its index, sd_at, drop_at, sd_max, the
                summary's order statistics (network_ref.box_stats) and the day records' selections -- and, from the
                kernel's own prob where given, expected (losses_ref.tree_sum) and expected_slots.  Without a prob it takes
                0.5 math.erfc(z 0.7071067811865476).

Everything is indexed by preorder position, as feeder_tree lays the nodes out; headroom_ref.to_pos / to_nodes convert."""
import math

import numpy as np

import network_ref as nr
from headroom_ref import to_nodes, to_pos  # noqa: F401  (re-exported)
from losses_ref import path_sums, tree_sum

INV_SQRT2 = 0.70710678118654752


def definition(R, s2, betas=()):
    """var (n, T) from the dense R (n, n), s2 (n, T) and the loadings betas (K, n, T)."""
    var = (R * R) @ s2
    for b in betas:
        var = var + (R @ b) ** 2
    return var


def flows(tree, x):
    """The flow scan: the subtree sums of x (n, T) by position."""
    C = np.concatenate([np.zeros((1, x.shape[1])), np.cumsum(x, 0)])
    return C[tree["end"]] - C[:-1]


def path_form(tree, w2, s2, betas=()):
    """-> (var, var_ind) (n, T) by position: s2 (n, T) and betas (K, n, T) by position, +0.0 where no row is."""
    terms = np.asarray(w2)[:, None] * flows(tree, s2)
    raw = path_sums(tree, terms)
    var_ind = np.where(raw > 0.0, raw, 0.0)
    var = var_ind
    for b in betas:
        c = path_sums(tree, np.asarray(tree["w"])[:, None] * flows(tree, b))
        var = var + c * c
    return var, var_ind


def prob_of(z):
    return np.array([[0.5 * math.erfc(v * INV_SQRT2) if not np.isnan(v) else np.nan for v in row] for row in np.atleast_2d(z)])


def contract(tree, n_nodes, sd, drop, drop_max, z_max, limit=None, out_mask=None, bad=None, prob=None):
    """sd, drop (and prob): (n, T) by position, the kernel's own.  limit / out_mask: (n,) bool by position or None (the
    positions with a row / all); bad: (T,) bool or None (no bad slot).
    -> dict(z, drop_q, prob (n, T) by position; slot: dict of (T,) arrays; summary: list of T dicts; day: dict of
    (n_nodes,) arrays in the caller's order; cov: the covered positions)."""
    n, T = drop.shape
    order = np.asarray(tree["order"], np.int64)
    has = order < n_nodes
    lim = (np.asarray(tree["src"]) >= 0) if limit is None else np.asarray(limit, bool)
    om = np.ones(n, bool) if out_mask is None else np.asarray(out_mask, bool)
    cov = has & lim & om
    bad = np.zeros(T, bool) if bad is None else np.asarray(bad, bool)
    slack = drop_max - drop
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0.0, slack / np.where(sd > 0.0, sd, 1.0), np.where(slack >= 0.0, np.inf, -np.inf))
    zs = z_max * sd
    drop_q = drop + zs
    z[:, bad], drop_q[:, bad] = np.nan, np.nan
    pr = prob_of(z) if prob is None else np.array(prob, np.float64)
    f8, i4 = lambda: np.full(T, np.nan), lambda v: np.full(T, v, np.int32)
    slot = dict(expected=f8(), z_min=f8(), sd_at=f8(), drop_at=f8(), sd_max=f8(), n_risky=i4(0), n_det=i4(0),
                z_min_index=i4(-1), n_bad=bad.astype(np.int32))
    summary = []
    pos = np.flatnonzero(cov)
    for t in range(T):
        if bad[t]:
            summary.append(dict(n_nan=int(cov.sum()), count=0, n_violations=0, worst_index=-1, worst_value=np.nan, box=None))
            continue
        slot["expected"][t] = tree_sum(np.where(cov, pr[:, t], 0.0))
        slot["n_risky"][t] = int((z[pos, t] < z_max).sum())
        slot["n_det"][t] = int((drop[pos, t] > drop_max).sum())
        if pos.size:
            zmin = z[pos, t].min()
            at = pos[z[pos, t] == zmin]
            j = int(at[np.argmin(order[at])])
            slot["z_min"][t], slot["z_min_index"][t] = zmin, order[j]
            slot["sd_at"][t], slot["drop_at"][t] = sd[j, t], drop[j, t]
            slot["sd_max"][t] = sd[pos, t].max()
        x, xi = drop_q[pos, t], order[pos]
        rec = dict(n_nan=0, count=int(x.size), n_violations=int((x > drop_max).sum()), worst_index=-1, worst_value=np.nan,
                   box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.max())
            rec["worst_index"] = int(xi[x == x.max()].min())
        summary.append(rec)
    # ---- the day of every node: by position, then in the caller's order
    pmax, zmin, exp = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    pslot, nrisky = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for j in range(n):
        for t in range(T):
            if bad[t]:
                continue
            p, v = pr[j, t], z[j, t]
            if pslot[j] < 0 or v < zmin[j]:
                zmin[j] = v
            if pslot[j] < 0 or p > pmax[j]:
                pmax[j], pslot[j] = p, t
            nrisky[j] += v < z_max
            exp[j] = exp[j] + p
    day = {}
    for k, a in (("prob_max", pmax), ("z_min", zmin), ("expected_slots", exp), ("prob_max_slot", pslot), ("n_risky", nrisky)):
        out = np.zeros(n_nodes, a.dtype)
        out[order[has]] = a[has]
        day[k] = out
    return dict(z=z, drop_q=drop_q, prob=pr, slot=slot, summary=summary, day=day, cov=cov)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_summary(got, want):
    """A device summary record array (T,) against contract()'s list: == for the order statistics and the counts, <= 2 ulp
    for the interpolated quartiles (test_gpu_network.check_summary's rule)."""
    for t, r in enumerate(want):
        g = got[t]
        assert (g["count"], g["n_nan"], g["n_violations"], g["worst_index"]) == \
            (r["count"], r["n_nan"], r["n_violations"], r["worst_index"]), (t, g, r)
        assert not g["reserved"].any()
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
