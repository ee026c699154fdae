"""Feeders that are not stars, for the tree-form kernels (csrc/tree_body.h), with inputs on grids that make every sum the
three prefix sums form exact in double whatever the order -- so a kernel is compared with an integer recursion bit for bit.

  forward grid   weighted_case(): w = 2 r integers 0..64 in 2^-6 (zeros included), injections integers 0..63 in 2^-4, junction
                 nodes, unchecked rows, rows off the tree, random node numbers (a parent may come after its child).
                 exact_voltages() walks the tree itself in Python integers -- leaves to roots for the flows, roots to leaves
                 for the voltages -- and shares nothing with revs_admm_amd.feeder.feeder_tree's preorder layout.
  inverse map    unit_tree(): every edge w = 1 (r = 0.5), every row a node; injections(forest, v) = flow - sum of the
                 children's flows with flow = v - v[parent] satisfies R p = v exactly for v on select_ref's 2^-10 grid: the
                 star-only bit-for-bit tests run on real trees with their expectations unchanged.  split > 0: that many
                 edges become two halves (w = 0.5 each) through a pass-through junction without a row -- what
                 feeder.tree_from_R inserts; the junction's voltage is the mean of its neighbours', on the 2^-11 grid.
numpy only (dense_R: the package's radial_R); tests/test_tree_cases.py holds both claims on the CPU."""
import functools

import numpy as np

from select_ref import G

KINDS = ("chain", "hub", "binary", "caterpillar", "comb")
P_BITS, W_BITS = 4, 6                       # the forward grid: p in 2^-4, w = 2 r in 2^-6; v in 2^-10 = select_ref.G


# ---- topologies: parent[] with parent[i] < i ------------------------------------------------------------------------
def chain(n):
    return np.arange(-1, n - 1, dtype=np.int64)


def hub(n):
    """one root, n - 1 leaves"""
    p = np.zeros(n, np.int64)
    p[0] = -1
    return p


def binary(n):
    p = (np.arange(n, dtype=np.int64) - 1) // 2
    p[0] = -1
    return p


def caterpillar(n):
    """a spine of (n + 1) // 2 nodes, one leaf on each (the last spine node of an odd n has none)"""
    s = (n + 1) // 2
    return np.concatenate([np.arange(-1, s - 1, dtype=np.int64), np.arange(n - s, dtype=np.int64)])


def comb(n, tooth=64):
    """a spine whose every node carries a chain of tooth - 1 (the last one what is left of n)"""
    i = np.arange(n, dtype=np.int64)
    return np.where(i % tooth == 0, i - tooth, i - 1).clip(min=-1)


def relabel(parent, rng):
    """the same tree under a random renumbering of its nodes: parent[i] > i occurs"""
    parent = np.asarray(parent, np.int64)
    perm = rng.permutation(len(parent))
    out = np.empty_like(parent)
    out[perm] = np.where(parent >= 0, perm[np.maximum(parent, 0)], -1)
    return out


def topology(kind, n, tooth=64):
    return comb(n, tooth) if kind == "comb" else {"chain": chain, "hub": hub, "binary": binary,
                                                  "caterpillar": caterpillar}[kind](n)


def _levels(parent):
    """the nodes parents first (breadth first from the roots: not a preorder)"""
    parent = np.asarray(parent, np.int64)
    kids = [[] for _ in parent]
    order = []
    for i, a in enumerate(parent):
        (order if a < 0 else kids[a]).append(i)
    k = 0
    while k < len(order):
        order.extend(kids[order[k]])
        k += 1
    assert len(order) == len(parent), "not a forest"
    return order


def dense_R(parent, edge_r):
    """the LinDistFlow matrix of a forest in ITS node numbers (synthetic.radial_R wants parents first)"""
    from revs_admm_amd.synthetic import radial_R
    parent, edge_r = np.asarray(parent, np.int64), np.asarray(edge_r, np.float64)
    order = np.asarray(_levels(parent))
    inv = np.empty(len(parent), np.int64)
    inv[order] = np.arange(len(parent))
    R = radial_R(np.where(parent[order] >= 0, inv[np.maximum(parent[order], 0)], -1), edge_r[order])
    return np.ascontiguousarray(R[np.ix_(inv, inv)])


# ---- the forward grid ------------------------------------------------------------------------------------------------
def exact_voltages(forest, checked, p, p_bits=P_BITS, w_bits=W_BITS):
    """(v float64[m][T], widest): R p at the rows with a checked position (0 elsewhere) for injections p[m][T] that are
    integers in 2^-p_bits on a forest whose 2 r are integers in 2^-w_bits -- in Python integers, by the tree itself:
    flow[i] = the injections of i's subtree (accumulated from the leaves to the roots), v[i] = v[parent[i]] + w[i] flow[i]
    (from the roots down).  Only rows that are checked inject.  widest: an integer no sum of these terms in ANY order
    exceeds, in units of 2^-(p_bits + w_bits) -- the largest of sum |injections| and sum_i w[i] |flow[i]|."""
    parent, edge_r, cons_of = (np.asarray(a) for a in forest)
    checked, p = np.asarray(checked, bool), np.asarray(p, np.float64)
    n, (m, T) = len(parent), p.shape
    pi = np.rint(p * 2.0 ** p_bits)
    wi = np.rint(2.0 * np.asarray(edge_r, np.float64) * 2.0 ** w_bits)
    assert np.array_equal(pi / 2.0 ** p_bits, p) and np.array_equal(wi / 2.0 ** (w_bits + 1), edge_r), "off the grid"
    has = (cons_of >= 0) & checked[np.maximum(cons_of, 0)]
    flow = [[int(x) for x in pi[cons_of[i]]] if has[i] else [0] * T for i in range(n)]
    wint = [int(x) for x in wi]
    order = _levels(parent)
    widest = max(sum(abs(f[t]) for f in flow) for t in range(T))
    for i in reversed(order):
        a = parent[i]
        if a >= 0:
            fa, fi = flow[a], flow[i]
            for t in range(T):
                fa[t] += fi[t]
    volt = [None] * n
    total = [0] * T
    for i in order:
        a, w, f = parent[i], wint[i], flow[i]
        up = volt[a] if a >= 0 else None
        volt[i] = [(up[t] if up else 0) + w * f[t] for t in range(T)]
        for t in range(T):
            total[t] += w * abs(f[t])
    widest = max(widest, max(total))
    v = np.zeros((m, T))
    unit = 2.0 ** -(p_bits + w_bits)
    for i in np.flatnonzero(has):
        v[cons_of[i]] = [x * unit for x in volt[i]]          # (below 2^53: the product with a power of two is exact)
    return v, widest


def _build_weighted(kind, n, seed, T):
    rng = np.random.default_rng([seed, n, T, KINDS.index(kind), 911])
    parent = relabel(topology(kind, n), rng)
    wq = rng.integers(0, 65, n)
    junction = rng.random(n) < 0.15
    if junction.all():
        junction[0] = False
    nr = int((~junction).sum())
    m = nr + 5                                               # (five rows without a position in the tree)
    cons_of = np.full(n, -1, np.int64)
    cons_of[~junction] = rng.permutation(m)[:nr]
    on = np.zeros(m, bool)
    on[cons_of[~junction]] = True
    checked = on & (rng.random(m) >= 0.15)
    if not checked.any():
        checked[np.flatnonzero(on)[0]] = True
    p = rng.integers(0, 64, (m, T)) / 16.0                   # (junk at unchecked rows and off the tree: never injected)
    y = np.zeros((m, T))
    rows = np.flatnonzero(checked)
    for t in range(T):
        r = rng.choice(rows, min(6, len(rows)), replace=False)
        y[r, t] = rng.integers(1, 64, len(r)) * np.where(rng.integers(0, 2, len(r)) == 1, 1, -1) / 16.0
    q = -rng.integers(0, 40, (m, T)) * G
    forest = (parent, wq / 128.0, cons_of)
    v, wide_p = exact_voltages(forest, checked, p)
    d, wide_y = exact_voltages(forest, checked, y)
    out = dict(kind=kind, n=n, T=T, m=m, forest=forest, wq=wq, on=on, checked=checked, p=p, y=y, q=q, v=v, d=d,
               widest=max(wide_p, wide_y))
    for a in list(out.values()) + list(forest):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def weighted_case(kind, n, seed=0, T=3):
    """One feeder of n nodes of `kind`, relabelled, on the forward grid: dict of forest = (parent, edge_r, cons_of) for
    feeder_tree, wq (edge_r = wq / 128), m rows, on (rows with a position), checked (a subset of `on`), p, y, q
    double[m][T], and v = R p, d = R y at the checked rows by exact_voltages (0 elsewhere); widest: see there.
    Read-only, computed once."""
    return _build_weighted(kind, n, seed, T)


def bounds(v, checked, lo=0.02, hi=0.97):
    """(vlo, vhi): the lo and hi quantiles of the distinct voltages at the checked rows, all slots together -- voltages
    themselves, hence on the 2^-10 grid, with rows AT each bound (not violated) and rows beyond each in some slot"""
    u = np.unique(v[checked])
    assert len(u) >= 3
    k_lo = min(max(int(lo * len(u)), 1), len(u) - 2)
    k_hi = max(min(int(hi * len(u)), len(u) - 2), k_lo)
    return float(u[k_lo]), float(u[k_hi])


def spread(c, m, seed=0):
    """weighted_case c with its rows scattered over m >= c["m"] rows (order kept): the added rows have no position in the
    tree, are unchecked, carry no multiplier and junk node sums."""
    rng = np.random.default_rng([seed, m, 913])
    to = np.sort(rng.permutation(m)[:c["m"]])
    parent, edge_r, cons_of = c["forest"]
    out = dict(c, m=m, forest=(parent, edge_r, np.where(cons_of >= 0, to[np.maximum(cons_of, 0)], -1)))
    for k in ("on", "checked"):
        out[k] = np.zeros(m, bool)
        out[k][to] = c[k]
    for k in ("y", "v", "d"):
        out[k] = np.zeros((m, c["T"]))
        out[k][to] = c[k]
    out["p"] = rng.integers(0, 64, (m, c["T"])) / 16.0
    out["p"][to] = c["p"]
    out["q"] = -rng.integers(0, 40, (m, c["T"])) * G
    out["q"][to] = c["q"]
    return out


# ---- the inverse map -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unit_tree(kind, M, split=0, seed=0, tooth=64):
    """(parent, edge_r, cons_of): M rows on a relabelled tree of `kind` whose every edge weighs w = 2 r = 1; row numbers
    are a random permutation of the nodes'.  split: that many edges (the substation's included) replaced by two halves
    through a junction node without a row -- M + split nodes."""
    rng = np.random.default_rng([seed, M, split, KINDS.index(kind), 912])
    parent = topology(kind, M, tooth)
    edge_r = np.full(M + split, 0.5)
    if split:
        cut = rng.choice(M, split, replace=False)
        parent = np.concatenate([parent, parent[cut]])       # junction M + s takes over the parent of cut[s] ...
        parent[cut] = M + np.arange(split)                   # ... and becomes it
        edge_r[cut] = 0.25
        edge_r[M:] = 0.25
    perm = rng.permutation(M + split)
    new = np.empty_like(parent)
    new[perm] = np.where(parent >= 0, perm[np.maximum(parent, 0)], -1)
    er = np.empty_like(edge_r)
    er[perm] = edge_r
    cons_of = np.full(M + split, -1, np.int64)
    cons_of[perm[:M]] = rng.permutation(M)
    for a in (new, er, cons_of):
        a.setflags(write=False)
    return new, er, cons_of


def injections(forest, v):
    """p double[M][T] with R p = v on a unit_tree: p = flow - sum of the children's flows, flow[i] = (v[i] - v[parent[i]]) /
    w[i] (the substation's voltage is 0).  A junction without a row sits at the mean of its two neighbours, so that it
    injects nothing.  Every operation is exact for v on the 2^-10 grid (w is 1 or 0.5)."""
    parent, edge_r, cons_of = (np.asarray(a) for a in forest)
    v = np.asarray(v, np.float64)
    n, T = len(parent), v.shape[1]
    vn = np.zeros((n + 1, T))                                # (slot n: the substation)
    row = cons_of >= 0
    vn[:n][row] = v[cons_of[row]]
    child = np.full(n, -1, np.int64)
    child[parent[parent >= 0]] = np.flatnonzero(parent >= 0)
    jun = np.flatnonzero(~row)
    assert (np.bincount(parent[parent >= 0], minlength=n)[jun] == 1).all(), "pass-through junctions only"
    assert row[child[jun]].all() and ((parent[jun] < 0) | row[np.maximum(parent[jun], 0)]).all()
    vn[jun] = 0.5 * (vn[parent[jun]] + vn[child[jun]])       # (parent -1 reads slot n)
    flow = (vn[:n] - vn[parent]) / (2.0 * edge_r)[:, None]
    out = flow.copy()
    np.subtract.at(out, parent[parent >= 0], flow[parent >= 0])
    assert np.abs(out[jun]).max(initial=0.0) == 0.0
    p = np.zeros_like(v)
    p[cons_of[row]] = out[row]
    return p


def tree_voltage_preorder_gather(tree, p):
    """feeder.tree_voltage_host with ONE thing wrong: the weighted flows are prefix-summed in preorder where the third
    scan wants them in end-order (eo taken as the identity).  The negative control of tests/test_tree_cases.py."""
    src = tree["src"]
    inj = np.where(src >= 0, 1.0, 0.0)[:, None] * p[np.maximum(src, 0)]
    C = np.concatenate([np.zeros((1, p.shape[1])), np.cumsum(inj, 0)])
    wp = tree["w"][:, None] * (C[tree["end"]] - C[:-1])
    pre = np.cumsum(wp, 0)
    F = np.concatenate([np.zeros((1, p.shape[1])), pre])
    v = pre - F[tree["cle"]]
    out = np.zeros_like(p)
    out[src[src >= 0]] = v[src >= 0]
    return out
