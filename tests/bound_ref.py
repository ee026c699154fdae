"""float64 numpy restatement of revs_dual_bound (include/revs_admm.h): the Lagrangian dual bound of the centralized
problem (oracle.solve_central_lp) at signed row multipliers y and scale s,
    L(s y) = sum_h min_{p_h in X_h} (c + s d[node(h)]).(LOAD_h + p_h) - s sum_{m,t} max(vhi y, vlo y),  d = R y.
Per residence: the window's slots ranked by r_t = c_t + s d[node][t], ties to the earlier slot (stable argsort);
relaxed chargers fill E* = clamp(rating #{r < 0}, E_lo, E_hi) at full rating in rank order, on/off chargers take the
n* = clamp(#{r < 0}, nmin, nmax) cheapest slots.  Residences whose own rows are empty are counted and left out."""
import numpy as np

SOC_TARGET, SOC_MAX = 0.9, 1.0


def dual_bound(cost, homes, load, node_of, R, y, scale, vlo, vhi, integral=False, d=None):
    """-> (bound, parts {home, load, row}, empty count, p* (N, T), node sums of p* (M, T)).  homes: HOME_DTYPE records,
    load (N, T), node_of (N,), R (M, M), y (M, T) or None.  d: R y when given (default R @ y)."""
    c = np.asarray(cost, np.float32).astype(np.float64)
    load = np.asarray(load, np.float64)
    N, T = load.shape
    M = R.shape[0]
    node_of = np.asarray(node_of, np.int64)
    if y is None:
        y = np.zeros((M, T))
        d = np.zeros((M, T))
    elif d is None:
        d = R.T @ y
    r = c[None, :] + scale * d[node_of]                              # (N, T)
    ev = homes["ev"] != 0
    t = np.arange(T)[None, :]
    win = ev[:, None] & (t >= homes["start"][:, None]) & (t < homes["end"][:, None])
    key = np.where(win, r, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(T)[None, :].repeat(N, 0), axis=1)
    nw = win.sum(1)
    nneg = (win & (r < 0)).sum(1)
    rt = homes["rating"].astype(np.float64)
    if integral:
        nmin, nmax = homes["nmin"].astype(np.int64), homes["nmax"].astype(np.int64)
        empty = ev & ((nmin > nmax) | (nmin > nw))
        ns = np.minimum(np.maximum(nneg, nmin), nmax)
        p = np.where(win & ~empty[:, None] & (rank < ns[:, None]), rt[:, None], 0.0)
    else:
        ini, cap = homes["initial"].astype(np.float64), homes["capacity"].astype(np.float64)
        elo = np.where(ev, (np.maximum(SOC_TARGET, ini) - ini) * cap, 0.0)
        ehi = np.where(ev, (SOC_MAX - ini) * cap, 0.0)
        empty = ev & ((elo > ehi) | (elo > rt * nw))
        es = np.minimum(np.maximum(rt * nneg, elo), ehi)
        p = np.where(win & ~empty[:, None], np.minimum(rt[:, None], np.maximum(0.0, es[:, None] - rank * rt[:, None])),
                     0.0)
    home = float((p * r).sum())
    lsum = np.zeros((M, T))
    np.add.at(lsum, node_of, load)
    load_part = float(((c[None, :] + scale * d) * lsum).sum())
    row = float(-scale * np.maximum(vhi * y, vlo * y).sum())
    pn = np.zeros((M, T))
    np.add.at(pn, node_of, p)
    return home + load_part + row, dict(home=home, load=load_part, row=row), int(empty.sum()), p, pn
