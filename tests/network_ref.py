"""float64 numpy restatement of the reference's dense network formulas (drawing.py:17-78) and of the box-plot numbers its
figures show: the yard-stick of the network report.  Nothing here knows the feeder is a tree.

    A      oriented incidence matrix of the non-substation nodes (networkx: -1 at an edge's first node, +1 at its second)
    flows  F = A^-1 P                         (compute_flows)
    R      2 Finv D Finv^T, Finv = (A^T)^-1   (compute_Rmat)
    V      sqrt(vset^2 - R P)                 (compute_voltage; NaN where the radicand is negative, as numpy gives)
    box    numpy.percentile (linear) and matplotlib.cbook.boxplot_stats' whisker rule at whis = 1.5"""
import numpy as np


def incidence(n_nodes, edge_u, edge_v, nonsub):
    A = np.zeros((n_nodes, len(edge_u)))
    A[edge_u, np.arange(len(edge_u))] = -1.0
    A[edge_v, np.arange(len(edge_u))] = 1.0
    return A[nonsub, :]


def dense(n_nodes, edge_u, edge_v, edge_r, nonsub):
    """-> (A_inv (edges x nodes), R (nodes x nodes)) over the non-substation nodes."""
    A = incidence(n_nodes, edge_u, edge_v, nonsub)
    A_inv = np.linalg.inv(A)
    Finv = np.linalg.inv(A.T)
    R = 2.0 * (Finv * np.asarray(edge_r, np.float64)[None, :]) @ Finv.T
    return A_inv, R


def flows(A_inv, P):
    return A_inv @ P


def volt(R, P, vset=1.0):
    with np.errstate(invalid="ignore"):
        return np.sqrt(vset * vset - R @ P)


def box_stats(x, whis=1.5):
    """matplotlib.cbook.boxplot_stats for one 1-d sample without NaNs -> dict, or None when it is empty."""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return None
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    iqr = q3 - q1
    loval, hival = q1 - whis * iqr, q3 + whis * iqr
    wlo = x[x >= loval]
    wlo = q1 if (wlo.size == 0 or wlo.min() > q1) else wlo.min()
    whi = x[x <= hival]
    whi = q3 if (whi.size == 0 or whi.max() < q3) else whi.max()
    return dict(min=x.min(), q1=q1, median=med, q3=q3, max=x.max(), whisker_lo=wlo, whisker_hi=whi,
                n_fliers=int(((x < wlo) | (x > whi)).sum()), count=int(x.size))


def summary(values, keep, kind, vmin=None, vmax=None):
    """The per-slot record of one quantity: values (entries, T); keep (entries,) bool: the rated lines / the nodes of
    interest; kind "loading" (violation: > 1, worst: the largest) or "volt" (violation: outside [vmin, vmax], worst:
    farthest outside -- or nearest to the edge of -- that band).  NaNs are counted and left out.  Lowest index on ties."""
    out = []
    idx = np.flatnonzero(keep)
    for t in range(values.shape[1]):
        col = values[idx, t]
        ok = ~np.isnan(col)
        x, xi = col[ok], idx[ok]
        rec = dict(n_nan=int((~ok).sum()), count=int(x.size), n_violations=0, worst_index=-1, worst_value=np.nan, box=box_stats(x))
        if x.size:
            if kind == "loading":
                rec["n_violations"] = int((x > 1.0).sum())
                key = x
            else:
                rec["n_violations"] = int(((x < vmin) | (x > vmax)).sum())
                key = np.maximum(vmin - x, x - vmax)
            j = int(np.flatnonzero(key == key.max())[np.argmin(xi[key == key.max()])])
            rec["worst_index"], rec["worst_value"] = int(xi[j]), float(x[j])
        out.append(rec)
    return out


def dense_solve(n_nodes, edge_u, edge_v, edge_r, nonsub, P):
    """(F, R P) = (A^-1 P, 2 (A^T)^-1 D A^-1 P) by one dense LU factorisation of A instead of two explicit inverses:
    the same dense formulas at the sizes (16 384 nodes) where forming R itself takes minutes."""
    from scipy.linalg import lu_factor, lu_solve
    lu = lu_factor(incidence(n_nodes, edge_u, edge_v, nonsub), overwrite_a=True, check_finite=False)
    F = lu_solve(lu, P, check_finite=False)
    RP = 2.0 * lu_solve(lu, np.asarray(edge_r, np.float64)[:, None] * F, trans=1, check_finite=False)
    return F, RP
