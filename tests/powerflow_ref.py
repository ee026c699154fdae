"""float64 numpy restatements of the power-flow report (include/revs_admm_ops.h, "power-flow report"), two of them:

  solve()     the fixed-point iteration of the header with numpy running sums in the scans' form (the flow scan as
              feeder.tree_report_host restates it, the path scan as losses_ref.path_sums), slot by slot, to a tol of
              choice or until it stalls; with every pass's max |du| and the contraction factor they show.
  contract()  from given volt, volt_lin, loss, inj (the kernel's own arrays) and the kernel's iters / status: every
              record in the header's exact order of operations -- the fixed binary tree of the sums, the box-plot record,
              the node days and the day.  (qloss_total is the one field it does not rebuild: lq is no output array.)

Everything is indexed by preorder position, as feeder_tree lays the nodes out; headroom_ref.to_pos / to_nodes convert."""
import numpy as np

import losses_ref as lr
import network_ref as nr


def flow_sums(tree, a):
    """The flow scan's form on the terms a (n,): C[end_j] - C[j], C the prefix in preorder."""
    C = np.concatenate([[0.0], np.cumsum(a)])
    return C[tree["end"]] - C[:-1]


def path_sums(tree, c):
    return lr.path_sums(tree, c[:, None])[:, 0]


def solve(tree, n_nodes, inj, vset2, xw=None, tan_phi=0.0, tol=1e-12, max_iter=32, stall=False, keep=False):
    """inj (n, T) by position; xw (n,) by position or None.  -> dict of (n, T) arrays u, P, Q, lp, lq, u_lin, P_lin and
    (T,) iters, status, rho; deltas: per slot the list of max |du| of the passes 1, 2, ...  stall=True: a slot also ends
    (status 0) behind the pass whose max |du| is 0 or no smaller than the pass before's while that is below 1e-12 vset2
    -- the iteration has reached the roundings of its own sums.  keep=True: hist, per slot the list of every pass's
    (u, P, Q, lp) behind pass 0."""
    n, T = inj.shape
    w = np.asarray(tree["w"], np.float64)
    has = np.asarray(tree["order"]) < n_nodes
    hasq = xw is not None
    x = np.asarray(xw, np.float64) if hasq else np.zeros(n)
    out = {k: np.full((n, T), np.nan) for k in ("u", "P", "Q", "lp", "lq", "u_lin", "P_lin")}
    iters, status, rho, deltas, hist = np.zeros(T, np.int32), np.zeros(T, np.int32), np.full(T, np.nan), [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(T):
            g = inj[:, t]
            q = tan_phi * g if hasq else np.zeros(n)
            P, Q = flow_sums(tree, g), (flow_sums(tree, q) if hasq else np.zeros(n))
            term = w * P
            if hasq:
                term = term + x * Q
            u = vset2 - path_sums(tree, term)
            out["u_lin"][:, t], out["P_lin"][:, t] = u, P
            lp, lq = np.zeros(n), np.zeros(n)
            ds, hs = [], []
            if not np.isfinite(g).all():
                status[t] = 1
            elif not (u[has] > 0.0).all():
                status[t] = 2
            k = 0
            while status[t] == 0:
                k += 1
                sq = P * P
                if hasq:
                    sq = sq + Q * Q
                cur = sq / u
                lp, lq = (0.5 * w) * cur, (0.5 * x) * cur
                P = flow_sums(tree, g + lp) - lp
                if hasq:
                    Q = flow_sums(tree, q + lq) - lq
                term = w * P
                if hasq:
                    term = term + x * Q
                h = w * lp
                if hasq:
                    h = h + x * lq
                term = term + 0.5 * h
                un = vset2 - path_sums(tree, term)
                d = np.abs(un - u)[has]
                d = np.nan if np.isnan(d).any() else d.max()
                u = un
                ds.append(d)
                iters[t] = k
                if keep:
                    hs.append((u, P, Q, lp))
                if not (u[has] > 0.0).all():
                    status[t] = 2
                    break
                if d <= tol * vset2:
                    break
                if stall and (d == 0.0 or (k >= 2 and d >= ds[-2] and ds[-2] < 1e-12 * vset2)):
                    break
                if k >= max_iter:
                    status[t] = 3
                    break
            deltas.append(ds)
            hist.append(hs)
            floor = 1e-13 * vset2                                  # (below it the ratios are those of rounding noise)
            r = [ds[i] / ds[i - 1] for i in range(1, len(ds)) if ds[i - 1] > floor]
            rho[t] = max(r) if r else 0.0
            if status[t] == 0:
                for k_, a in (("u", u), ("P", P), ("Q", Q), ("lp", lp), ("lq", lq)):
                    out[k_][:, t] = a
    out.update(iters=iters, status=status, rho=rho, deltas=deltas, hist=hist)
    return out


def contract(tree, n_nodes, volt, volt_lin, loss, inj, iters, status, vmin, node_mask=None, cost=None, slot_hours=1.0):
    """volt, volt_lin, loss, inj: (n, T) by position; iters, status: (T,), the kernel's; node_mask: (n,) bool by position
    or None (all).  -> dict(slot: dict of (T,) arrays, summary: list of T dicts, node_day: dict of (n_nodes,) arrays in the
    caller's order, day: dict)."""
    n, T = volt.shape
    order = np.asarray(tree["order"], np.int64)
    has = order < n_nodes
    nm = has & (np.ones(n, bool) if node_mask is None else np.asarray(node_mask, bool))
    bad = np.asarray(status) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        loss_total = lr.tree_sum(np.where(has[:, None] & ~bad[None, :], loss, 0.0))
        delivered = lr.tree_sum(inj)
        supplied = delivered + loss_total
    for a in (loss_total, delivered, supplied):
        a[bad] = np.nan
    vmin_v, vmin_i = np.full(T, np.nan), np.full(T, -1, np.int32)
    err_v, err_i = np.full(T, np.nan), np.full(T, -1, np.int32)
    nb, nbl, nms = (np.zeros(T, np.int32) for _ in range(3))
    pos = np.flatnonzero(nm)
    summary = []
    for t in range(T):
        v, vl = volt[pos, t], volt_lin[pos, t]
        if not bad[t] and pos.size:
            lo = v.min()
            vmin_v[t], vmin_i[t] = lo, order[pos][v == lo].min()
            with np.errstate(invalid="ignore"):
                e = vl - v
                okk = ~np.isnan(e)
                if okk.any():
                    top = e[okk].max()
                    err_v[t], err_i[t] = top, order[pos][okk & (e == top)].min()
                b, bl = v < vmin, vl < vmin
            nb[t], nbl[t], nms[t] = b.sum(), bl.sum(), (b & ~bl).sum()
        ok = ~np.isnan(v)
        x, xi = v[ok], order[pos][ok]
        rec = dict(n_nan=int((~ok).sum()), count=int(x.size), n_violations=int((x < vmin).sum()), worst_index=-1,
                   worst_value=np.nan, box=nr.box_stats(x))
        if x.size:
            rec["worst_value"] = float(x.min())
            rec["worst_index"] = int(xi[x == x.min()].min())
        summary.append(rec)
    slot = dict(loss_total=loss_total, delivered=delivered, supplied=supplied, volt_min=vmin_v, err_max=err_v,
                volt_min_index=vmin_i, err_index=err_i, n_below=nb, n_below_lin=nbl, n_missed=nms,
                iters=np.asarray(iters, np.int32), status=np.asarray(status, np.int32))
    # ---- the day of every node: by position, then in the caller's order
    dmin, dslot = np.full(n, np.nan), np.full(n, -1, np.int32)
    dbel, dmis = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for j in np.flatnonzero(has):
        for t in range(T):
            v, vl = volt[j, t], volt_lin[j, t]
            if np.isnan(v):
                continue
            if dslot[j] < 0 or v < dmin[j]:
                dmin[j], dslot[j] = v, t
            dbel[j] += v < vmin
            dmis[j] += (v < vmin) and not (vl < vmin)
    node_day = {}
    for k, a in (("volt_min", dmin), ("slot", dslot), ("slots_below", dbel), ("slots_missed", dmis)):
        o = np.zeros(n_nodes, a.dtype)
        o[order[has]] = a[has]
        node_day[k] = o
    # ---- the day of the scenario
    e = d = co = 0.0
    day = dict(volt_min=np.nan, volt_min_slot=-1, volt_min_index=-1, n_below=0, n_below_lin=0, n_missed=0, iters_max=0,
               n_bad_slots=int(bad.sum()))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            e = e + loss_total[t]
            d = d + delivered[t]
            if cost is not None:
                co = co + loss_total[t] * float(cost[t])
            if vmin_i[t] >= 0 and (day["volt_min_slot"] < 0 or vmin_v[t] < day["volt_min"]):
                day.update(volt_min=vmin_v[t], volt_min_slot=t, volt_min_index=int(vmin_i[t]))
            day["n_below"] += int(nb[t])
            day["n_below_lin"] += int(nbl[t])
            day["n_missed"] += int(nms[t])
            day["iters_max"] = max(day["iters_max"], int(iters[t]))
        day.update(energy_lost=e * slot_hours, energy_delivered=d * slot_hours,
                   cost=co * slot_hours if cost is not None else np.nan)
    return dict(bad=bad, slot=slot, summary=summary, node_day=node_day, day=day)
