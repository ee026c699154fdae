"""The folded chain's operator launch (include/revs_admm_ops.h: revs_op_chain_kv; csrc/newton_kernels.hip:
op_chain_kv_kernel): inputs that take every branch of it, and a plain float64 numpy restatement of one launch.

On top of tests/select_ref.py (the 2^-10 grid, restate(), star_forest()).  The kernel takes the feeder twice, and the two
are independent in it: as a TREE for the row voltages, and as the dense R for the Gram sums and the shifts.
  tree      star_forest: the tree form of R p is p, so rows, sums, lists and stats are exact and numpy gives them bit for bit;
            or (TREES) a chain, a comb, a comb with split edges from tests/tree_cases.py: every edge w = 1 (two halves
            through a junction where split), random node numbers, and p = the injections whose tree form is v -- as exact;
  dense R   m x m, multiples of 2^-4 with |r| < 2 (zeros included); N integers 0..16 (zeros included); kappa = 4: every
            Gram sum over up to 2048 nodes is below 2^17 at resolution 2^-8 -- exact in double in any order -- so K from
            chain_fast_body, from small_model_body and from numpy agree bit for bit (tests/test_chain_cases.py checks the
            claim in integers).
One column (slot) per scenario, T = 24 (NAMES).  The multipliers of a column are the outcome of a step from a PREVIOUS list
-- what select_ref.restate() leaves for a prior state whose multipliers are the list's head and whose violated rows are
its tail -- so "every row with a multiplier is on the previous list" holds by construction.  Where a count does not fit a
small M the column holds what fits.  numpy only."""
import functools

import numpy as np

import select_ref as sr
import tree_cases as tc
from select_ref import BAND, G, T, VHI, VLO

A = 128                                   # REVS_DUAL_AMAX
KADD, KAPPA, DELTA, MAX_PIVOTS, SCALE, EPS = 16, 4.0, 1e-10, 300, VHI, 1e-8
KADD_PREV = 8                             # of the prior state's selection: the previous lists hold at most 8 + 8 rows
NAMES = ("empty", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "unsorted_support", "not_same", "leaving", "neg_zero",
         "mult_on_violated", "at_bound", "no_step", "nine", "many", "prev9", "prev_overflow", "nv256", "nv257",
         "ties_one_thread", "ends")
assert len(NAMES) == T
SIZES = (1, 9, 255, 257, 2048)            # rows = tree rows; 2048 = REVS_CHAIN_FOLD_MAX_M: the launch's LDS is over 64 KB
# name -> (rows with a position in the tree, rows m, junction nodes without a row)
GEOMETRY = {**{str(M): (M, M, 0) for M in SIZES}, "off_tree": (257, 300, 0), "junctions": (255, 255, 10),
            "chain255": (255, 255, 0), "chain2048": (2048, 2048, 0), "comb255": (255, 255, 0), "comb2048": (2048, 2048, 0),
            # (2038 rows on the tree: with the ten junctions its 2048 positions are all the launch holds)
            "split_edges255": (255, 255, 10), "split_edges2048": (2038, 2048, 10)}
# the geometries on a real tree -- the others are forests of roots --: name -> (kind of tree_cases.unit_tree, split edges)
TREES = {"chain255": ("chain", 0), "chain2048": ("chain", 0), "comb255": ("comb", 0), "comb2048": ("comb", 0),
         "split_edges255": ("comb", 10), "split_edges2048": ("comb", 10)}


class _Col:
    """One column under construction, in the numbering of the rows that have a position in the tree."""

    def __init__(self, rng, M):
        self.rng, self.M = rng, M
        self.k = rng.integers(-BAND + 1, BAND, M)        # strictly inside the band: nothing at a bound by accident
        self.y = np.zeros(M)
        self.head, self.tail, self.used = [], [], set()  # the previous list: rows with a multiplier then | added then
        self.pool = [int(r) for r in rng.permutation(M)]
        self.prev_overflow = False
        self.sparse_n = None                             # (leaving: the rows whose Gram entries are kept small)

    def take(self, n, rows=None):
        """up to n rows nobody has taken (from `rows` in that order, else at random): what fits"""
        out = []
        for r in (self.pool if rows is None else rows):
            if len(out) == n:
                break
            if 0 <= r < self.M and r not in self.used:
                out.append(int(r))
                self.used.add(int(r))
        return out

    def support(self, rows, where="head", push=None, y=None):
        """multipliers on `rows` (non-zero integers, |y| <= 8), each row `push` grid steps beyond its own bound"""
        for i, r in enumerate(rows):
            yv = float(self.rng.integers(1, 9) * (1 if self.rng.integers(0, 2) else -1)) if y is None else float(y[i])
            d = int(self.rng.integers(-3, 4)) if push is None else int(push[i] if np.ndim(push) else push)
            self.y[r] = yv
            self.k[r] = BAND + d if yv > 0 else -BAND - d
        (self.head if where == "head" else self.tail).extend(rows)

    def violate(self, rows, steps, side=None):
        rows, steps = list(rows), np.asarray(steps)
        side = sr._side(self.rng, len(rows)) if side is None else side
        self.k[rows] = side * (BAND + (steps[:len(rows)] if steps.ndim else steps))


def _a(A_, variant):
    """a1..a8: exactly A_ candidates; the split between support and added rows turns with the size"""
    def fill(c):
        ns = (0, A_, A_ // 2, A_ - 1)[(A_ + variant) % 4]
        rows = c.take(ns)
        ntail = min(len(rows), A_ % 3)              # the last ones were ADDED rows of the step before: not in row order
        c.support(rows[:len(rows) - ntail])
        c.support(rows[len(rows) - ntail:], where="tail")
        if A_ % 2 == 0 and len(rows) < 8:
            c.head.extend(c.take(1))                # a row whose multiplier the step before took to zero
        add = c.take(A_ - len(rows))
        c.violate(add, c.rng.integers(1, 30, len(add)))
    return fill


def _unsorted_support(c):
    M = c.M
    c.support(c.take(2, [M - 2, M - 4]))
    c.support(c.take(2, [3, 1]), where="tail")      # added by the step before, below the head, larger row first
    c.violate(c.take(1), 12)


def _not_same(c):
    M = c.M
    c.support(c.take(2, [M - 3, M - 2]), push=0, y=[3.0, -2.0])
    c.violate(c.take(2, [1, 2]), [30, 20])          # enter below the support: list order is no longer row order


def _leaving(c):
    rows = c.take(2)
    c.support(rows[:1], push=-100, y=[1.0])         # far inside its bound with a small multiplier: the model drops it
    c.support(rows[1:], push=0, y=[3.0])
    c.sparse_n = rows


def _neg_zero(c):
    r = c.take(1)
    c.head.extend(r)                                # on the previous list, and the step before left it at -0.0
    c.violate(r, 9)
    c.y[r] = -0.0
    c.support(c.take(2))
    c.violate(c.take(1), 5)


def _mult_on_violated(c):
    rows = c.take(3)
    c.support(rows)
    c.violate(rows, 50)                             # (side drawn independently of the sign of y)
    c.violate(c.take(3), [40, 50, 60])


def _at_bound(c):
    c.support(c.take(2), push=0)
    at = c.take(4)
    c.k[at] = sr._side(c.rng, len(at)) * BAND       # AT the bound: not violated
    c.violate(c.take(2), 1)


def _prev9(c):
    rows = c.take(9)
    c.support(rows[:3])
    c.head.extend(rows[3:])
    c.violate(c.take(2), [7, 7])


def _prev_overflow(c):
    c.support(c.take(4))
    c.violate(c.take(2), [4, 9])
    c.prev_overflow = True


def _nv(nvw):
    def fill(c):
        rows = c.take(nvw)
        c.violate(rows, c.rng.integers(1, 6, len(rows)))
        c.support(c.take(2))                        # (what is left: at M = 257 one row beside 256, none beside 257)
    return fill


def _ties_one_thread(c):
    own = c.take(8, range(8, 16)) + c.take(8, range(5, c.M, 256))     # a thread's eight positions | a thread's strided rows
    c.violate(own, 150)
    oth = c.take(30)
    c.violate(oth, c.rng.integers(1, 21, len(oth)))


def _ends(c):
    c.violate(c.take(2, [0, c.M - 1]), 120)
    c.support(c.take(2, [1, c.M - 2]))
    c.violate(c.take(2), [3, 8])


def _fills(variant):
    f = {"empty": lambda c: None, "unsorted_support": _unsorted_support, "not_same": _not_same, "leaving": _leaving,
         "neg_zero": _neg_zero, "mult_on_violated": _mult_on_violated, "at_bound": _at_bound,
         "no_step": lambda c: c.support(c.take(3), push=0),
         "nine": lambda c: (c.support(c.take(5)), c.violate(c.take(4), [2, 9, 9, 4])),
         "many": lambda c: (c.support(c.take(8)), c.violate(c.take(40), c.rng.integers(1, 30, 40))),
         "prev9": _prev9, "prev_overflow": _prev_overflow, "nv256": _nv(256), "nv257": _nv(257),
         "ties_one_thread": _ties_one_thread, "ends": _ends}
    f.update({f"a{k}": _a(k, variant) for k in range(1, 9)})
    return [f[n] for n in NAMES]


def build(name, seed=0):
    """One launch's inputs for GEOMETRY[name]: dict of m, the forest (parent, edge_r, cons_of) of feeder_tree, `on` (rows
    with a position), v (the row voltages the tree form gives: zero off the tree), y, pnq double[3][m][T] (p | N | q:
    junk off the tree), R, prev_cidx / prev_ccnt."""
    M, m, njun = GEOMETRY[name]
    variant = list(GEOMETRY).index(name)
    rng = np.random.default_rng([seed, M, m, 4242])
    cons = np.sort(rng.permutation(m)[:M]).astype(np.int64)         # (monotone: row order is kept)
    on = np.zeros(m, bool)
    on[cons] = True
    R = rng.integers(-31, 32, (m, m)) * (rng.integers(0, 4, (m, m)) > 0) / 16.0
    R[np.arange(m), np.arange(m)] = np.where(np.diag(R) == 0, 5 / 16.0, np.diag(R))
    N = rng.integers(0, 17, (m, T)).astype(np.float64)
    k, y = np.zeros((m, T), np.int64), np.zeros((m, T))
    k0, y0 = np.zeros((m, T), np.int64), np.zeros((m, T))
    overflow = []
    for t, fill in enumerate(_fills(variant)):
        c = _Col(rng, M)
        fill(c)
        k[cons, t], y[cons, t] = c.k, c.y
        used = cons[sorted(c.used)]
        N[used, t] = np.maximum(N[used, t], 1.0)                    # (no candidate row without curvature of its own)
        if c.sparse_n:                                              # leaving: curvature at one or two nodes only
            i = cons[c.sparse_n[0]]
            nz = np.flatnonzero(R[i])
            N[:, t] = 0.0
            N[nz[np.argmin(np.abs(R[i, nz]))], t] = 1.0
            if len(c.sparse_n) > 1:
                j = cons[c.sparse_n[1]]
                only_j = np.flatnonzero((R[i] == 0) & (R[j] != 0))
                N[only_j[:1] if len(only_j) else j, t] = 2.0
        # the prior state that leaves this column's previous list: multipliers on the head, violated rows in the tail's order
        assert len(c.tail) <= KADD_PREV and len(set(c.head) | set(c.tail)) == len(c.head) + len(c.tail)
        k0[cons, t] = rng.integers(-BAND + 1, BAND, M)
        y0[cons[c.head], t] = 1.0
        k0[cons[c.tail], t] = BAND + len(c.tail) - np.arange(len(c.tail))
        if c.prev_overflow:
            overflow.append(t)
    prev = sr.restate(k0 * G, y0, np.zeros((3, m, T)), VLO, VHI, KADD_PREV, A)
    prev_cidx, prev_ccnt = prev["cidx"].copy(), prev["ccnt"].copy()
    prev_cidx[overflow], prev_ccnt[overflow] = 0, -1                # (what a selection leaves of more than 128 multipliers)
    junk = rng.integers(-255, 256, (m, T))
    p = np.where(on[:, None], k, junk) * G
    q = -rng.integers(0, 40, (m, T)) * G
    if name in TREES:
        # a real tree: row r of unit_tree is row cons[r] here, and the node sums are the injections that give v
        parent, edge_r, rows = tc.unit_tree(*((TREES[name][0], M, TREES[name][1])))
        assert (rows < 0).sum() == njun
        p[cons] = tc.injections((parent, edge_r, rows), (k * G)[cons])
        forest = (parent, edge_r, np.where(rows >= 0, cons[np.maximum(rows, 0)], -1))
    else:
        # the forest: every row's node hangs off the substation by an edge of resistance 0.5, junction nodes in between
        cons_of = np.concatenate([cons, np.full(njun, -1, np.int64)])[rng.permutation(M + njun)] if njun else cons
        forest = (np.full(len(cons_of), -1, np.int64), np.full(len(cons_of), 0.5), cons_of)
    out = dict(name=name, m=m, forest=forest, on=on, v=np.where(on[:, None], k * G, 0.0), y=y,
               pnq=np.ascontiguousarray(np.stack([p, N, q])), R=np.ascontiguousarray(R), prev_cidx=prev_cidx,
               prev_ccnt=prev_ccnt)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


def _solve_models(m, R, N, sel, kappa, delta, max_pivots):
    """yhat double[T][A], info int32[T] by tests/fake_kernels.py's block principal pivoting (its rule and tolerances, not a
    copy of them); a column of more than 8 candidates is left where it is and flagged -999, as the small model does."""
    from fake_kernels import FakeKernels
    nt = len(sel["ccnt"])
    small = (sel["ccnt"] >= 1) & (sel["ccnt"] <= 8)
    ccnt = np.where(small, sel["ccnt"], 0).astype(np.int32)         # (no candidates: yhat = the multipliers, info = 0)
    cidx, cval = np.ascontiguousarray(sel["cidx"]), np.ascontiguousarray(sel["cval"])
    Rc, Nc = np.ascontiguousarray(R), np.ascontiguousarray(N)
    yhat, info = np.zeros((nt, A)), np.zeros(nt, np.int32)
    FakeKernels().revs_op_dual_model_small(m, nt, Rc.ctypes.data, Nc.ctypes.data, cidx.ctypes.data, ccnt.ctypes.data,
                                           cval.ctypes.data, kappa, delta, max_pivots, None, yhat.ctypes.data,
                                           info.ctypes.data, None)
    info[sel["ccnt"] > 8] = -999
    return yhat, info


def shifts(R, rows, yv, kappa):
    """sum_k R[rows[k]][.] yv[k] / kappa, the terms in the order given (float64)"""
    d = np.zeros(R.shape[1])
    for r, v in zip(rows, yv):
        d = d + R[r] * v
    return d / kappa


def restate_chain(v, y, pnq, R, vlo=VLO, vhi=VHI, kadd=KADD, kappa=KAPPA, delta=DELTA, max_pivots=MAX_PIVOTS, scale=SCALE,
                  eps=EPS):
    """What one launch's step half leaves for row voltages v[m][T], multipliers y, node terms pnq and the dense R:
    select_ref.restate's outputs (rows and selection), K double[T][A][A] (the candidates' Gram block, zero elsewhere),
    yhat, info, alpha, y_trial, lin double[T], sh_a / sh_b double[T][m] and, per column, pc-independent counts: ns, nv,
    cnt, `same` (the rows with a multiplier after the step ascend in list order: sh_b is sh_a), tr (the trace of K)."""
    v, y, R = np.asarray(v, np.float64), np.asarray(y, np.float64), np.asarray(R, np.float64)
    m, nt = v.shape
    N = np.asarray(pnq)[1]
    out = sr.restate(v, y, pnq, vlo, vhi, kadd, A)
    cnt = np.maximum(out["ccnt"], 0)
    K = np.zeros((nt, A, A))
    for t in range(nt):
        a = cnt[t] if cnt[t] <= 8 else 0
        RF = R[out["cidx"][t, :a]]
        K[t, :a, :a] = (RF * N[:, t][None, :]) @ RF.T / kappa
    yhat, info = _solve_models(m, R, N, out, kappa, delta, max_pivots)
    alpha = (out["sums"][:, 0] / scale > eps).astype(np.float64)
    y_trial, lin = y.copy(), np.zeros(nt)
    sh_a, sh_b, same = np.zeros((nt, m)), np.zeros((nt, m)), np.ones(nt, bool)
    for t in range(nt):
        a, rows = cnt[t], out["cidx"][t, :cnt[t]]
        yo = out["cval"][t, 2, :a]
        yn = yhat[t, :a] if alpha[t] == 1.0 else yo
        y_trial[rows, t] = yn
        lin[t] = (out["cval"][t, 1, :a] * (yn - yo)).sum()
        sh_a[t] = shifts(R, rows, yn, kappa)
        carry = rows[yn != 0]
        same[t] = a > 8 or bool((np.diff(carry) > 0).all())     # (more than 8: the kernel keeps list order for both)
        sh_b[t] = sh_a[t] if same[t] else shifts(R, np.sort(carry), yn[yn != 0][np.argsort(carry)], kappa)
    out.update(K=K, yhat=yhat, info=info, alpha=alpha, y_trial=y_trial, lin=lin, sh_a=sh_a, sh_b=sh_b, same=same,
               ns=out["sums"][:, 2].astype(int), nv=out["sums"][:, 3].astype(int), cnt=cnt,
               tr=np.einsum("tii->t", K))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    pnq = c["pnq"].copy()                       # (off the tree: no voltage, no dual term; N counts in the Gram sums)
    pnq[0], pnq[2] = c["v"], np.where(c["on"][:, None], c["pnq"][2], 0.0)
    out = restate_chain(c["v"], c["y"], pnq, c["R"])
    for a in out.values():
        a.setflags(write=False)
    return out


def path(c, e, t, es=4, prev=True):
    """Which predicates of op_chain_kv_kernel slot t satisfies, from the restatement's own counts: the set of
    'ranked' (chain_rows_select_body publishes the lists) or 'general' (tree_rows_body + dual_select_body), then
    'empty' | 'fast<A>' (with 'npre=0' | 'npre=A' | 'npre<A', 'ns>=5', 'same' | 'not_same') | 'over8'."""
    pc, ns, nv, cnt = int(c["prev_ccnt"][t]), int(e["ns"][t]), int(e["nv"][t]), int(e["cnt"][t])
    ranked = prev and es == 4 and c["m"] <= 2048 and 0 <= pc <= 8 and nv <= 256
    s = {"ranked" if ranked else "general"}
    if cnt == 0:
        s.add("empty")
    elif cnt <= 8:
        npre = ns if ranked else 0
        s |= {f"fast<{cnt}>", "npre=0" if npre == 0 else ("npre=A" if npre == cnt else "npre<A"),
              "same" if e["same"][t] else "not_same"}
        if ns >= 5:
            s.add("ns>=5")
        if e["alpha"][t] == 0.0:
            s.add("no_step")
    else:
        s.add("over8")
    return s


def lcp_ok(e, t, yh, delta=DELTA):
    """Whether yh (a model answer for slot t of the restatement e, at most 8 candidates) satisfies the LCP of the model:
    the conditions and the tolerance of tests/test_gpu_newton.py: test_model_problem_sizes."""
    a = int(e["cnt"][t])
    s, grad, ycur = e["cval"][t, 0, :a], e["cval"][t, 1, :a], e["cval"][t, 2, :a]
    K0 = e["K"][t, :a, :a]
    Kp = K0 * s[:, None] * s[None, :] + (delta * np.trace(K0) / a) * np.eye(a)
    c = s * grad + Kp @ np.maximum(s * ycur, 0.0)
    u = s * np.asarray(yh)[:a]
    w = Kp @ u - c
    tol = 1e-8 * (np.abs(Kp).sum(axis=1).max() * max(u.max(), 1e-300) + np.abs(c).max())
    return bool(u.min() >= 0.0 and w.min() >= -tol and np.abs(w[u > 0]).max(initial=0.0) <= tol
                and (np.asarray(yh)[a:] == 0).all())
