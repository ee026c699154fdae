"""float64 numpy restatements of the headroom report (include/revs_admm_ops.h, "headroom report"), two of them:

  definition()  (a) the all-pairs definition: x[i] = max(0, min over the limit nodes j with R[i][j] > 0 of s[j] / R[i][j],
                min over the rated lines a on i's root path of rating[a] - flow[a]) from a dense R and the lines of every
                root path.  Nothing in it knows about subtrees.
  contract()    (b) the contract, level by level: the subtree minima going up, the path minima with their limiter going
                down (a strict < keeps the shallowest, the voltage term goes before the thermal one), then summary()
                (network_ref.box_stats) and day().

Everything is indexed by preorder position, as feeder_tree lays the nodes out; to_pos / to_nodes convert."""
import numpy as np

import network_ref as nr


def to_pos(tree, a, fill=0.0):
    """(nodes, ...) in the caller's node order -> (tree n, ...) by position; padding positions get `fill`."""
    a = np.asarray(a)
    order = np.asarray(tree["order"])
    real = order < a.shape[0]
    out = np.full((len(order),) + a.shape[1:], fill, a.dtype)
    out[real] = a[order[real]]
    return out


def to_nodes(tree, a, n_nodes):
    """(tree n, ...) by position -> (n_nodes, ...) in the caller's node order."""
    order = np.asarray(tree["order"])
    real = order < n_nodes
    out = np.zeros((n_nodes,) + a.shape[1:], a.dtype)
    out[order[real]] = a[real]
    return out


def lca_matrix(parent_pos, depth, wc):
    """R[i][j] = wc[lca(i, j)] (0 where i and j share no ancestor) by a naive walk: of the two, the deeper one steps
    to its parent until they meet.  One row at a time, the walk of all j against i side by side."""
    n = len(parent_pos)
    par = np.append(np.asarray(parent_pos, np.int64), -1)          # (par[-1] = -1: the substation stays where it is)
    dep = np.append(np.asarray(depth, np.int64), -1)
    wcx = np.append(np.asarray(wc, np.float64), 0.0)
    R = np.zeros((n, n))
    for i in range(n):
        a, b = np.full(n, i, np.int64), np.arange(n, dtype=np.int64)
        while True:
            diff = a != b
            if not diff.any():
                break
            up_a = diff & (dep[a] >= dep[b])
            up_b = diff & (dep[b] > dep[a])
            a = np.where(up_a, par[a], a)
            b = np.where(up_b, par[b], b)
        R[i] = wcx[a]
    return R


def root_paths(parent_pos):
    """The lines on every root path: path[i] = [i, parent(i), ...]."""
    out = []
    for i in range(len(parent_pos)):
        p, j = [], i
        while j >= 0:
            p.append(j)
            j = int(parent_pos[j])
        out.append(p)
    return out


def definition(R, paths, limit, drop, flow, rating, drop_max):
    """(a): headroom (n, T) by position."""
    n, T = drop.shape
    s = drop_max - drop
    x = np.full((n, T), np.inf)
    lim = np.flatnonzero(limit)
    rated = rating > 0
    for i in range(n):
        js = lim[R[i, lim] > 0]
        if len(js):
            x[i] = np.minimum(x[i], (s[js] / R[i, js][:, None]).min(axis=0))
        ls = [a for a in paths[i] if rated[a]]
        if ls:
            x[i] = np.minimum(x[i], (rating[ls][:, None] - flow[ls]).min(axis=0))
    return np.where(x > 0.0, x, 0.0)


def contract(aux, limit, drop, flow, rating, drop_max, nan_slot=None):
    """(b): (headroom (n, T), limiter position (n, T) or -1, kind (n, T) or -1) by position.  nan_slot: (T,) bool, the
    slots whose injections are not finite: every headroom a NaN, every limiter -1."""
    parent, wc, depth = (np.asarray(aux[k]) for k in ("parent_pos", "wc", "depth"))
    n, T = drop.shape
    levels = [np.flatnonzero(depth == d) for d in range(int(depth.max(initial=0)) + 1)]
    A = np.where(np.asarray(limit, bool)[:, None], drop_max - drop, np.inf)
    for lev in levels[:0:-1]:                                  # up: every node after all of its children
        np.minimum.at(A, parent[lev], A[lev])
    with np.errstate(divide="ignore", invalid="ignore"):
        volt = np.where(wc[:, None] > 0, A / np.where(wc > 0, wc, 1.0)[:, None], np.inf)
    thr = np.where((rating > 0)[:, None], np.where(rating > 0, rating, 0.0)[:, None] - flow, np.inf)
    thermal = ~(volt <= thr)                                   # (the voltage term first on a tie)
    val = np.where(thermal, thr, volt)
    q, at = val.copy(), np.tile(np.arange(n)[:, None], (1, T))
    for lev in levels[1:]:                                     # down: every node after its parent
        p = parent[lev]
        keep = q[p] <= val[lev]                                # (a strict < moves the limiter: the shallowest stays)
        q[lev] = np.where(keep, q[p], val[lev])
        at[lev] = np.where(keep, at[p], at[lev])
    kind = np.take_along_axis(thermal, at, axis=0).astype(np.int32)
    none = np.isinf(q) & (q > 0)
    head = np.where(q > 0.0, q, 0.0)
    at, kind = np.where(none, -1, at), np.where(none, -1, kind)
    if nan_slot is not None and np.any(nan_slot):
        head[:, nan_slot], at[:, nan_slot], kind[:, nan_slot] = np.nan, -1, -1
    return head, at, kind


def limiter_words(tree, at, kind, n_nodes):
    """limiter_out's words by position: node | kind << 30, -1 unlimited."""
    order = np.asarray(tree["order"])
    node = order[np.maximum(at, 0)]
    return np.where((at < 0) | (node >= n_nodes), -1, node | (kind << 30)).astype(np.int32)


def summary(head_nodes, keep, need):
    """The per-slot records of headrooms (nodes, T) in the caller's node order over the nodes with keep."""
    out = []
    idx = np.flatnonzero(keep)
    for t in range(head_nodes.shape[1]):
        col = head_nodes[idx, t]
        fin = np.isfinite(col)
        x, xi = col[fin], idx[fin]
        rec = dict(n_nan=int(np.isnan(col).sum()), n_unlimited=int((col == np.inf).sum()), count=int(x.size),
                   n_violations=int((x < need).sum()), worst_index=-1, worst_value=np.nan, box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.min())
            rec["worst_index"] = int(xi[x == x.min()].min())
        out.append(rec)
    return out


def day(head_nodes, need):
    """(min, slot, n_short) per node over the slots that are no NaN."""
    n, T = head_nodes.shape
    mn, slot, short = np.full(n, np.nan), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        for t in range(T):
            v = head_nodes[i, t]
            if np.isnan(v):
                continue
            if slot[i] < 0 or v < mn[i]:
                mn[i], slot[i] = v, t
            short[i] += v < need
    return mn, slot, short
