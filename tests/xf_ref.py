"""float64 numpy restatement of the transformer report (include/revs_admm_ops.h, "transformer report"), operation by
operation: every operation that is no pow / exp is one IEEE double operation (numpy never fuses), pow is numpy.power and
exp numpy.exp.  load, ratio and everything computed from them alone are therefore the kernel's bits; top_oil, hot_spot and
faa differ from the kernel's by what two pow / exp implementations may differ (propagated_bounds), so the records that
are computed from them are restated from GIVEN hot / faa arrays (restate(hot=, faa=): the kernel's own), the loss tests'
contract() idiom.

All arrays are (K, T); the recursion runs over the slots and sub-steps for all transformers at once."""
import numpy as np

import network_ref as nr

MODEL = dict(dto_r=55.0, dhs_r=25.0, loss_ratio=5.0, n=0.8, m=0.8, aging_B=15000.0, theta_ref=110.0,
             normal_life_hours=180000.0)
U = 2.0 ** -53                       # unit roundoff: one rounded operation moves a value by at most U |value|


def decays(slot_hours, q, tau_to=3.0, tau_w=0.08):
    h = slot_hours / q
    return float(np.exp(-h / tau_to)), (float(np.exp(-h / tau_w)) if tau_w > 0 else 0.0)


def csr(members):
    """members: a list of row lists -> (xf_ptr, xf_rows)"""
    ptr = np.zeros(len(members) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in members])
    return ptr, np.array([r for rows in members for r in rows], np.int32)


def grouped(g, xf_ptr, xf_rows, rated_kw):
    """-> (load (K, T): the rows' sums from +0.0 in list order, a row outside 0..m-1 adding nothing; bad (K,))"""
    m, T = g.shape
    K = len(xf_ptr) - 1
    load, bad = np.zeros((K, T)), np.zeros(K, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            acc = np.zeros(T)
            for j in range(max(int(xf_ptr[k]), 0), min(int(xf_ptr[k + 1]), len(xf_rows))):
                row = int(xf_rows[j])
                if 0 <= row < m:
                    acc = acc + g[row]
                    bad[k] |= not np.isfinite(g[row]).all()
                else:
                    bad[k] = True
            load[k] = acc
    rated_kw = np.asarray(rated_kw, np.float64)
    bad |= ~(np.isfinite(rated_kw) & (rated_kw > 0.0))
    return load, bad


def recursion(u_to, u_w, ambient, mdl, q, decay_to, decay_w, cyclic, to0, w0):
    """-> dict(top_oil, hot, faa (K, T); x0, y0, x_end, y_end (K,))"""
    K, T = u_to.shape
    B = mdl["aging_B"]
    c0 = B / (mdl["theta_ref"] + 273.0)
    with np.errstate(all="ignore"):
        if cyclic:
            x, y, aN, awN = np.zeros(K), np.zeros(K), 1.0, 1.0
            for t in range(T):
                for _ in range(q):
                    x = u_to[:, t] + (x - u_to[:, t]) * decay_to
                    y = u_w[:, t] + (y - u_w[:, t]) * decay_w
                    aN, awN = aN * decay_to, awN * decay_w
            x, y = x / (1.0 - aN), y / (1.0 - awN)
        else:
            x, y = np.full(K, float(to0)), np.full(K, float(w0))
        x0, y0 = x.copy(), y.copy()
        top, hot, faa = np.zeros((K, T)), np.zeros((K, T)), np.zeros((K, T))
        for t in range(T):
            acc = np.zeros(K)
            for _ in range(q):
                x = u_to[:, t] + (x - u_to[:, t]) * decay_to
                y = u_w[:, t] + (y - u_w[:, t]) * decay_w
                h = (ambient[t] + x) + y
                acc = acc + np.exp(c0 - B / (h + 273.0))
            top[:, t], hot[:, t], faa[:, t] = x, h, acc / float(q)
    return dict(top_oil=top, hot=hot, faa=faa, x0=x0, y0=y0, x_end=x, y_end=y)


def first_peak(a):
    """(the largest value of each row, its earliest slot): a later slot replaces the peak only when strictly larger."""
    K, T = a.shape
    pk, at = a[:, 0].copy(), np.zeros(K, np.int32)
    for t in range(1, T):
        up = a[:, t] > pk
        pk[up], at[up] = a[up, t], t
    return pk, at


def slot_sum(a):
    acc = np.zeros(a.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(a.shape[1]):
            acc = acc + a[:, t]
    return acc


def tree_sum(x):
    """The root of the fixed binary tree over x, padded with +0.0 to the next power of two."""
    x = np.asarray(x, np.float64)
    size = 1
    while size < x.shape[0]:
        size *= 2
    y = np.zeros(size)
    y[:x.shape[0]] = x
    with np.errstate(invalid="ignore", over="ignore"):
        while y.shape[0] > 1:
            y = y[0::2] + y[1::2]
    return float(y[0])


def box_summary(values, limit):
    """Per slot the record over the K transformers: NaNs counted and left out, the worst the largest value and the lowest
    transformer that has it."""
    out = []
    for t in range(values.shape[1]):
        col = values[:, t]
        ok = ~np.isnan(col)
        x, xi = col[ok], np.flatnonzero(ok)
        with np.errstate(invalid="ignore"):
            box = nr.box_stats(x)
        rec = dict(n_nan=int((~ok).sum()), count=int(x.size), n_violations=int((x > limit).sum()), worst_index=-1,
                   worst_value=np.nan, box=box)
        if x.size:
            rec["worst_value"] = float(x.max())
            rec["worst_index"] = int(xi[x == x.max()].min())
        out.append(rec)
    return out


def restate(g, xf_ptr, xf_rows, rated_kw, ambient, mdl=MODEL, slot_hours=1.0, q=1, decay_to=None, decay_w=None, cyclic=1,
            to0=0.0, w0=0.0, over_ratio=1.0, hot_limit=110.0, hot=None, faa=None):
    """One scenario: g (m, T).  hot / faa: (K, T) arrays to restate the records from instead of this module's own (a bad
    transformer's rows of them must be NaN, as the kernel leaves them).  -> dict(load, ratio, bad, u_to, u_w, top_oil,
    hot, faa, x0, y0, x_end, y_end, day: dict of (K,) arrays, summary_ratio / summary_hot: lists of T dicts, fleet)."""
    g = np.asarray(g, np.float64)
    T = g.shape[1]
    rated_kw, ambient = np.asarray(rated_kw, np.float64), np.asarray(ambient, np.float64)
    if decay_to is None:
        decay_to, decay_w = decays(slot_hours, q)
    load, bad = grouped(g, xf_ptr, xf_rows, rated_kw)
    R = mdl["loss_ratio"]
    with np.errstate(all="ignore"):
        ratio = np.abs(load) / rated_kw[:, None]
        r2 = ratio * ratio
        u_to = mdl["dto_r"] * np.power((r2 * R + 1.0) / (R + 1.0), mdl["n"])
        u_w = mdl["dhs_r"] * np.power(r2, mdl["m"])
    rec = recursion(u_to, u_w, ambient, mdl, q, decay_to, decay_w, cyclic, to0, w0)
    for k in ("top_oil", "hot", "faa"):
        rec[k][bad] = np.nan
    use_hot = rec["hot"] if hot is None else np.asarray(hot, np.float64)
    use_faa = rec["faa"] if faa is None else np.asarray(faa, np.float64)
    with np.errstate(all="ignore"):
        pr, prs = first_peak(ratio)
        ph, phs = first_peak(use_hot)
        energy = slot_sum(np.abs(load)) * slot_hours
        age = slot_sum(use_faa) * slot_hours
        lol = 100.0 * age / mdl["normal_life_hours"]
        feqa = age / (float(T) * slot_hours)
        n_over = (ratio > over_ratio).sum(axis=1).astype(np.int32)
        n_hot = (use_hot > hot_limit).sum(axis=1).astype(np.int32)
    for a in (pr, ph, energy, age, lol, feqa):
        a[bad] = np.nan
    for a in (prs, phs):
        a[bad] = -1
    n_over[bad], n_hot[bad] = 0, 0
    day = dict(peak_ratio=pr, peak_hot=ph, energy_kwh=energy, age_hours=age, lol_percent=lol, feqa=feqa,
               peak_ratio_slot=prs, peak_hot_slot=phs, n_over_slots=n_over, n_hot_slots=n_hot)
    K = len(rated_kw)
    cand = sorted((-lol[k], k) for k in range(K) if not np.isnan(lol[k]))[:8]
    with np.errstate(all="ignore"):
        fleet = dict(n_xf=K, n_nan=int(np.isnan(lol).sum()), n_overloaded=int((n_over > 0).sum()), n_hot=int((n_hot > 0).sum()),
                     n_aging=int((feqa > 1.0).sum()), lol_sum=tree_sum(lol), energy_kwh=tree_sum(energy),
                     feqa_mean=tree_sum(age) / ((float(K) * float(T)) * slot_hours),
                     top_index=np.array([k for _, k in cand] + [-1] * (8 - len(cand)), np.int32),
                     top_lol=np.array([-v for v, _ in cand] + [np.nan] * (8 - len(cand))))
    fleet["lol_max"] = fleet["top_lol"][0]
    return dict(rec, load=load, ratio=ratio, bad=bad, u_to=u_to, u_w=u_w, day=day, fleet=fleet,
                summary_ratio=box_summary(ratio, over_ratio), summary_hot=box_summary(use_hot, hot_limit))


def propagated_bounds(r, ambient, mdl, q, decay_to, decay_w, cyclic, E=16.0):
    """How far top_oil, hot_spot and faa of an implementation of the contract may lie from restate()'s -> (b_top, b_hot,
    b_faa), each (K, T) (NaN rows where the transformer is bad).

    Both implementations see the same bits of ratio, so the same arguments of the two pow.  Each is within d of the
    contract evaluated in exact arithmetic, and the bound between them is 2 d, with d carried as follows (U = 2^-53;
    a pow / exp result is within E ulp <= 2 E U of the true value):
      u_to, u_w   the pow and one product: (2 E + 1) U |u|
      a sub-step  x' = u + (x - u) decay moves an incoming error ex to decay ex + (1 - decay) eu <= decay ex + eu -- the
                  recursion contracts with factor decay -- and adds three roundings, each at most U times an operand of
                  size <= 2 X with X the largest |u| or |start|: 6 U X
      cyclic      x0 = x_end / (1 - aN): the first pass' error over (1 - aN), the product aN's T q roundings
                  (T q U aN / (1 - aN) relative) and the subtraction and division (4 U |x0|)
      hot         ex + ey + two sums: 3 U (|ambient| + |x| + |y|)
      exponent    a = c0 - B / (hot + 273): c0's two roundings 2 U c0, the denominator D = hot + 273 within eD = eh + U D,
                  so B / D within B eD / (D (D - eD)) + U B / D, and the difference's rounding U |a|
      exp         exp(a) (2 E U + expm1(ea)); acc's q additions and the division by q: (q + 1) U faa."""
    u_to, u_w = r["u_to"], r["u_w"]
    K, T = u_to.shape
    B = mdl["aging_B"]
    c0 = B / (mdl["theta_ref"] + 273.0)
    amb = np.abs(np.asarray(ambient, np.float64))

    def chain(u, decay, start):
        eu = (2.0 * E + 1.0) * U * np.abs(u)
        X = np.maximum(np.abs(u).max(axis=1), np.abs(start))

        def steps(e):
            out = []
            for t in range(T):
                for _ in range(q):
                    e = decay * e + eu[:, t] + 6.0 * U * X
                    out.append(e)
            return out

        e0 = np.zeros(K)
        if cyclic:
            aN = decay ** (T * q)
            e0 = steps(np.zeros(K))[-1] / (1.0 - aN) + np.abs(start) * (4.0 * U + T * q * U * aN / (1.0 - aN))
        return np.array(steps(e0)).reshape(T, q, K)            # the error after every sub-step

    with np.errstate(all="ignore"):
        ex, ey = chain(u_to, decay_to, r["x0"]), chain(u_w, decay_w, r["y0"])
        # the sub-steps' states again, for the sizes the roundings scale with
        x, y = r["x0"].copy(), r["y0"].copy()
        b_top, b_hot, b_faa = np.zeros((K, T)), np.zeros((K, T)), np.zeros((K, T))
        for t in range(T):
            eacc = np.zeros(K)
            for s in range(q):
                x = u_to[:, t] + (x - u_to[:, t]) * decay_to
                y = u_w[:, t] + (y - u_w[:, t]) * decay_w
                h = (ambient[t] + x) + y
                eh = ex[t, s] + ey[t, s] + 3.0 * U * (amb[t] + np.abs(x) + np.abs(y))
                D = h + 273.0
                eD = eh + U * np.abs(D)
                assert (D - eD > 0.0)[~r["bad"]].all()
                a = c0 - B / D
                ea = 2.0 * U * c0 + B * eD / (D * (D - eD)) + U * B / D + U * np.abs(a)
                eacc = eacc + np.exp(a) * (2.0 * E * U + np.expm1(ea))
            b_top[:, t], b_hot[:, t] = ex[t, q - 1], eh
            b_faa[:, t] = eacc / q + (q + 1.0) * U * r["faa"][:, t]
    for b in (b_top, b_hot, b_faa):
        b *= 2.0
        b[r["bad"]] = np.nan
    return b_top, b_hot, b_faa
