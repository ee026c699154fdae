"""float64 numpy restatements of the loss report (include/revs_admm_ops.h, "loss report"), two of them:

  definition()  from dense F and R P (network_ref.dense_solve) and the lines of every root path: den, loss, c, and mlf as
                the sum of c along each root path (math.fsum: the exact sum, rounded once).  Nothing in it knows about
                scans or fixed trees.
  contract()    from given flow and drop (the kernel's own flow_out / drop_out, or tree_report_host's): the exact order
                of operations of the header, the fixed binary tree of the sums, the box-plot record, the day loops and
                the top 8.  mlf is the one quantity whose bits depend on the launch shape (a block scan): contract()
                computes it with numpy's running sums in the drop scan's form, and takes the kernel's own mlf instead
                (mlf=) where the slot record's mlf_max is to be compared bit for bit.

Everything is indexed by preorder position, as feeder_tree lays the nodes out; headroom_ref.to_pos / to_nodes convert."""
import math

import numpy as np

import network_ref as nr


def parent_positions(tree):
    """Position of every position's parent, -1 below the substation (read off `end`, as feeder.headroom_aux does)."""
    n, end = int(tree["n"]), np.asarray(tree["end"], np.int64)
    parent, stack = np.full(n, -1, np.int64), []
    for j in range(n):
        while stack and end[stack[-1]] <= j:
            stack.pop()
        if stack:
            parent[j] = stack[-1]
        stack.append(j)
    return parent


def root_paths(parent_pos):
    out = []
    for i in range(len(parent_pos)):
        p, j = [], i
        while j >= 0:
            p.append(j)
            j = int(parent_pos[j])
        out.append(p)
    return out


def definition(w, F, RP, vset2, paths):
    """-> dict(den, loss, c, mlf), each (n, T) by position, from the dense flows F and drops R P by position."""
    w = np.asarray(w, np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = vset2 - RP
        loss = 0.5 * w * F * F / den
        c = w * F / den
    mlf = np.array([[math.fsum(c[p, t]) for t in range(c.shape[1])] for p in paths]) if c.shape[1] else np.zeros_like(c)
    return dict(den=den, loss=loss, c=c, mlf=mlf)


def tree_sum(x):
    """The root of the fixed binary tree over the rows of x (n, ...): padded with +0.0 to the next power of two, then
    level by level x[i] = x[2i] + x[2i + 1]."""
    x = np.asarray(x, np.float64)
    size = 1
    while size < x.shape[0]:
        size *= 2
    y = np.zeros((size,) + x.shape[1:])
    y[:x.shape[0]] = x
    while y.shape[0] > 1:
        y = y[0::2] + y[1::2]
    return y[0]


def path_sums(tree, c):
    """The drop scan's form on the terms c (n, T): the prefix in preorder minus the prefix in end-order below cle."""
    pre = np.cumsum(c, 0)
    F = np.concatenate([np.zeros((1, c.shape[1])), np.cumsum(c[tree["eo"]], 0)])
    return pre - F[tree["cle"]]


def contract(tree, n_nodes, flow, drop, inj, vset2, line_mask=None, node_mask=None, line_class=None, C=0,
             loss_max=np.inf, cost=None, slot_hours=1.0, mlf=None):
    """flow, drop, inj: (n, T) by position.  line_mask / node_mask: (n,) bool by position or None (all); line_class:
    (n,) integers by position or None.  mlf: (n, T) by position to take instead of the numpy path sums (NaN rows of a
    bad slot included or not: they are overwritten).  -> dict(loss, mlf, c, den (n, T) by position; bad (T,);
    slot: dict of (T,) arrays; summary: list of T dicts; line_day: dict of (n_nodes,) arrays in the caller's order;
    day: dict)."""
    n, T = flow.shape
    order = np.asarray(tree["order"], np.int64)
    w = np.asarray(tree["w"], np.float64)[:, None]
    has = order < n_nodes
    lm = has & (np.ones(n, bool) if line_mask is None else np.asarray(line_mask, bool))
    nm = has & (np.ones(n, bool) if node_mask is None else np.asarray(node_mask, bool))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = vset2 - drop
        loss = ((0.5 * w) * flow) * flow / den
        c = (w * flow) / den
        bad = ~np.isfinite(inj).all(axis=0) | (~(den > 0.0) & has[:, None]).any(axis=0)
        ml = path_sums(tree, c) if mlf is None else np.array(mlf, np.float64)
        total = tree_sum(np.where(lm[:, None], loss, 0.0))
        delivered = tree_sum(inj)
        cls = np.zeros((4, T))
        for k in range(C):
            cls[k] = tree_sum(np.where((np.asarray(line_class) == k)[:, None], loss, 0.0))
    loss[:, bad], ml[:, bad] = np.nan, np.nan
    total[bad], delivered[bad], cls[:, bad] = np.nan, np.nan, np.nan
    mmax, mix = np.full(T, np.nan), np.full(T, -1, np.int32)
    for t in range(T):
        sel = nm & ~np.isnan(ml[:, t])
        if bad[t] or not sel.any():
            continue
        top = ml[sel, t].max()
        at = np.flatnonzero(sel & (ml[:, t] == top))
        j = at[np.argmin(order[at])]
        mmax[t], mix[t] = ml[j, t], order[j]
    slot = dict(total=total, delivered=delivered, class_total=cls.T.copy(), mlf_max=mmax, mlf_max_index=mix,
                n_bad=bad.astype(np.int32))
    # ---- the box-plot record of the summarised lines' losses
    summary = []
    pos = np.flatnonzero(lm)
    for t in range(T):
        col = loss[pos, t]
        ok = ~np.isnan(col)
        x, xi = col[ok], order[pos][ok]
        rec = dict(n_nan=int((~ok).sum()), count=int(x.size), n_violations=int((x > loss_max).sum()), worst_index=-1,
                   worst_value=np.nan, box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.max())
            rec["worst_index"] = int(xi[x == x.max()].min())
        summary.append(rec)
    # ---- the day of every line: by position, then in the caller's order
    energy, peak, pslot = np.zeros(n), np.zeros(n), np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            acc = 0.0
            for t in range(T):
                v = loss[j, t]
                acc = acc + v
                if pslot[j] < 0 or v > peak[j]:
                    peak[j], pslot[j] = v, t
            energy[j] = acc * slot_hours
    if bad.any():
        peak[:], pslot[:] = np.nan, -1
    line_day = {}
    for k, a in (("energy", energy), ("peak", peak), ("peak_slot", pslot)):
        out = np.zeros(n_nodes, a.dtype)
        out[order[has]] = a[has]
        line_day[k] = out
    # ---- the day of the scenario
    e = d = co = 0.0
    ce = [0.0] * 4
    pk, pk_at = 0.0, -1
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            e = e + total[t]
            d = d + delivered[t]
            for k in range(4):
                ce[k] = ce[k] + cls[k, t]
            if cost is not None:
                co = co + total[t] * float(cost[t])
            if pk_at < 0 or total[t] > pk:
                pk, pk_at = total[t], t
        day = dict(energy=e * slot_hours, delivered=d * slot_hours, class_energy=np.array(ce) * slot_hours,
                   cost=co * slot_hours if cost is not None else np.nan, peak=np.nan if bad.any() else pk,
                   peak_slot=-1 if bad.any() else pk_at, n_bad_slots=int(bad.sum()))
    cand = [(-(energy[j]), int(order[j])) for j in np.flatnonzero(lm) if not np.isnan(energy[j])]
    cand.sort()
    top = cand[:8]
    day["top_index"] = np.array([i for _, i in top] + [-1] * (8 - len(top)), np.int32)
    day["top_energy"] = np.array([-v for v, _ in top] + [np.nan] * (8 - len(top)))
    return dict(loss=loss, mlf=ml, c=c, den=den, bad=bad, slot=slot, summary=summary, line_day=line_day, day=day)


def propagated_bounds(w, F, RP, vset2, paths, rel=1e-12):
    """What a flow within eF = rel max|F| and a drop within eD = rel max|R P| of the dense ones (the bounds the network
    report's scans are held to) can move: -> (bound on |loss - definition's|, on |c - definition's|, on |mlf -
    definition's|), each (n, T).  loss = 0.5 w F^2 / den moves by at most 0.5 w (2 |F| eF + eF^2) / (den - eD) through
    the flow and loss eD / (den - eD) through the denominator, plus the four roundings of the expression; c = w F / den
    likewise; mlf by its path's bounds on c plus 2 n 2^-53 sum |c| for the order of its sum."""
    w = np.asarray(w, np.float64)[:, None]
    u = 2.0 ** -53
    eF, eD = rel * np.abs(F).max(), rel * np.abs(RP).max()
    den = vset2 - RP
    lo = den - eD
    assert (lo > 0).all()
    loss, c = 0.5 * w * F * F / den, w * F / den
    b_loss = 0.5 * w * (2.0 * np.abs(F) * eF + eF * eF) / lo + np.abs(loss) * eD / lo + 8 * u * np.abs(loss)
    b_c = w * eF / lo + np.abs(c) * eD / lo + 8 * u * np.abs(c)
    b_mlf = np.array([b_c[p].sum(axis=0) for p in paths]) + 2.0 * len(paths) * u * np.abs(c).sum(axis=0)[None, :]
    return b_loss, b_c, b_mlf
