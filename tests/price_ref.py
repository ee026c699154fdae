"""float64 numpy restatements of the price report (include/revs_admm_ops.h, "price report"), two of them:

  walk()      the two scans by parent walk: flow[j] = the sum of x over j's subtree, accumulated child into parent in
              reverse preorder, and drop[j] = drop[parent(j)] + w[j] flow[j], parents first.  Nothing in it knows about
              prefix sums; its order of additions is its own, so it is compared with the dense R y to a bound, not bit
              for bit.
  contract()  from given scans (the kernel's own flow_out / drop_out / line_y_out and, taken from a call with s = 1 and
              cost = 1, d = cong_out and mlf = lossp_out; or walk()'s): the exact order of operations of the header, the
              fixed binary tree of the sums (losses_ref.tree_sum), the box-plot record, the day loops and the top 8.

Everything is indexed by preorder position, as feeder_tree lays the nodes out; headroom_ref.to_pos / to_nodes convert."""
import numpy as np

import losses_ref as lr
import network_ref as nr


def walk(tree, x):
    """x (n, T) by position -> (flow, drop) by position, by parent walk."""
    parent = lr.parent_positions(tree)
    w = np.asarray(tree["w"], np.float64)
    flow = np.array(x, np.float64)
    for j in range(len(parent) - 1, -1, -1):
        if parent[j] >= 0:
            flow[parent[j]] += flow[j]
    drop = w[:, None] * flow
    for j in range(len(parent)):
        if parent[j] >= 0:
            drop[j] += drop[parent[j]]
    return flow, drop


def gathered(tree, rows):
    """rows (M, T) -> (n, T) by position: the row the position carries, +0.0 without one."""
    src = np.asarray(tree["src"])
    return np.where((src >= 0)[:, None], np.asarray(rows, np.float64)[np.maximum(src, 0)], 0.0)


def _argbest(vals, sel, order):
    """(value, caller index) of the largest vals over sel, ties to the lowest caller index; (NaN, -1) when none."""
    sel = sel & ~np.isnan(vals)
    if not sel.any():
        return np.nan, -1
    top = vals[sel].max()
    at = np.flatnonzero(sel & (vals == top))
    j = at[np.argmin(order[at])]
    return vals[j], int(order[j])


def contract(tree, n_nodes, flow, drop, line_y, d, mlf, inj, mu, s, cost, vset2=1.0, with_loss=True, line_mask=None,
             node_mask=None, slot_hours=1.0, price_cap=np.inf):
    """flow, drop, line_y, d, mlf, inj, mu: (n, T) by position (mlf: NaN rows of a bad slot are overwritten; ignored
    without with_loss).  s: the scenario's scale; cost: (T,).  line_mask / node_mask: (n,) bool by position or None.
    -> dict(price, cong, lossp, rent (n, T) by position; bad (T,); slot: dict of (T,) arrays; summary: list of T dicts;
    node_day, line_day: dicts of (n_nodes,) arrays in the caller's order; day: dict)."""
    n, T = flow.shape
    order = np.asarray(tree["order"], np.int64)
    w = np.asarray(tree["w"], np.float64)[:, None]
    cost = np.asarray(cost, np.float64)
    has = order < n_nodes
    lm = has & (np.ones(n, bool) if line_mask is None else np.asarray(line_mask, bool))
    nm = has & (np.ones(n, bool) if node_mask is None else np.asarray(node_mask, bool))
    s = np.float64(s)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        bad = ~np.isfinite(inj).all(axis=0) | ~np.isfinite(mu).all(axis=0) | ~(np.isfinite(s) and s >= 0.0)
        if with_loss:
            bad = bad | (~((vset2 - drop) > 0.0) & has[:, None]).any(axis=0)
            lossp = cost[None, :] * np.array(mlf, np.float64)
        else:
            lossp = np.zeros((n, T))
        cong = s * d
        price = (cost[None, :] + lossp) + cong
        rent = ((w * line_y) * flow) * s + 0.0
        pl, pc, pp = inj * lossp, inj * cong, inj * price
        delivered = lr.tree_sum(inj)
        energy_pay = cost * delivered
        loss_pay = lr.tree_sum(np.where(nm[:, None], pl, 0.0))
        cong_pay = lr.tree_sum(np.where(nm[:, None], pc, 0.0))
        rent_total = lr.tree_sum(np.where(lm[:, None], rent, 0.0))
    for a in (price, cong, lossp, rent, pp, pc):
        a[:, bad] = np.nan
    for a in (delivered, energy_pay, loss_pay, cong_pay, rent_total):
        a[bad] = np.nan
    slot = dict(delivered=delivered, energy_pay=energy_pay, loss_pay=loss_pay, cong_pay=cong_pay, rent_total=rent_total,
                n_bad=bad.astype(np.int32))
    for k in ("price_max", "price_min", "cong_max"):
        slot[k], slot[k + "_index"] = np.full(T, np.nan), np.full(T, -1, np.int32)
    slot["n_priced"], slot["n_rows"] = np.zeros(T, np.int32), np.zeros(T, np.int32)
    for t in range(T):
        if bad[t]:
            continue
        slot["price_max"][t], slot["price_max_index"][t] = _argbest(price[:, t], nm, order)
        v, slot["price_min_index"][t] = _argbest(-price[:, t], nm, order)
        slot["price_min"][t] = -v
        slot["cong_max"][t], slot["cong_max_index"][t] = _argbest(cong[:, t], nm, order)
        slot["n_priced"][t] = int((nm & (cong[:, t] != 0.0)).sum())
        slot["n_rows"][t] = int((mu[:, t] != 0.0).sum())
    # ---- the box-plot record of the summarised nodes' prices
    summary = []
    pos = np.flatnonzero(nm)
    for t in range(T):
        col = price[pos, t]
        ok = ~np.isnan(col)
        x, xi = col[ok], order[pos][ok]
        rec = dict(n_nan=int((~ok).sum()), count=int(x.size), n_violations=int((x > price_cap).sum()), worst_index=-1,
                   worst_value=np.nan, box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.max())
            rec["worst_index"] = int(xi[x == x.max()].min())
        summary.append(rec)
    # ---- the day of every node and of every line: by position, then in the caller's order
    def day_of(vals, sums):
        acc = [np.zeros(n) for _ in sums]
        peak, pslot = np.zeros(n), np.full(n, -1, np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(T):
                for a, x in zip(acc, sums):
                    a += x[:, t]
                v = vals[:, t]
                take = (pslot < 0) | (v > peak)
                peak, pslot = np.where(take, v, peak), np.where(take, t, pslot).astype(np.int32)
            anynan = np.isnan(vals).any(axis=1)
            return [a * slot_hours for a in acc], np.where(anynan, np.nan, peak), np.where(anynan, -1, pslot).astype(np.int32)

    def to_nodes(a):
        out = np.zeros(n_nodes, a.dtype)
        out[order[has]] = a[has]
        return out

    (paid, cpaid), ppeak, pslot = day_of(price, (pp, pc))
    (renergy,), rpeak, rslot = day_of(rent, (rent,))
    node_day = dict(paid=to_nodes(paid), cong_paid=to_nodes(cpaid), peak_price=to_nodes(ppeak), peak_slot=to_nodes(pslot))
    line_day = dict(energy=to_nodes(renergy), peak=to_nodes(rpeak), peak_slot=to_nodes(rslot))
    # ---- the day of the scenario
    tot = dict(energy_pay=0.0, loss_pay=0.0, cong_pay=0.0, rent_total=0.0)
    pk, pk_at, pk_ix = 0.0, -1, -1
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            for k in tot:
                tot[k] = tot[k] + slot[k][t]
            if slot["price_max_index"][t] >= 0 and (pk_at < 0 or slot["price_max"][t] > pk):
                pk, pk_at, pk_ix = slot["price_max"][t], t, int(slot["price_max_index"][t])
        day = {k: v * slot_hours for k, v in tot.items()}
    none = bad.any() or pk_at < 0
    day.update(peak_price=np.nan if none else pk, peak_slot=-1 if none else pk_at, peak_index=-1 if none else pk_ix,
               n_bad_slots=int(bad.sum()), n_cong_slots=int((slot["n_rows"] > 0).sum()))
    cand = [(-(renergy[j]), int(order[j])) for j in np.flatnonzero(lm) if not np.isnan(renergy[j])]
    cand.sort()
    top = cand[:8]
    day["top_index"] = np.array([i for _, i in top] + [-1] * (8 - len(top)), np.int32)
    day["top_rent"] = np.array([-v for v, _ in top] + [np.nan] * (8 - len(top)))
    return dict(price=price, cong=cong, lossp=lossp, rent=rent, bad=bad, slot=slot, summary=summary, node_day=node_day,
                line_day=line_day, day=day)
