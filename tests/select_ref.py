"""Candidate-row selection of the operator's dual Newton path: inputs on a grid and a plain float64 numpy restatement
of what a rows kernel plus the selection leave (include/revs_admm_ops.h: revs_op_dual_select, revs_op_dual_select_big).

Everything lies on the 2^-10 grid: vhi = 64 g, vlo = -vhi, v = k g with |k| < 2^8, multipliers non-zero integers with
|y| <= 8, the dual terms q minus small integers times g.  Every quantity the kernels form from them -- violations,
gradients v - bound, vhi y, the sum of 16384 dual terms -- is then exact in double whatever the order of summation, so
a kernel is compared with restate() bit for bit, and equal violations (the tie rule: larger first, lower row first)
arise by themselves.  numpy only; tests/fake_kernels.py is NOT used here: tests/test_select_ref.py holds the two
writings of the rule against each other."""
import functools

import numpy as np

G = 2.0 ** -10
BAND = 64                     # vhi = BAND * G
VHI, VLO = BAND * G, -BAND * G
T = 24
KMAX = 255                    # |k| < 2^8: the largest violation is KMAX - BAND = 191 grid steps


def _inside(rng, M):
    """k of M rows inside the band (bounds included: a row AT its bound is not violated)."""
    return rng.integers(-BAND, BAND + 1, M)


def _side(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, 1, -1)


def _mult(rng, n):
    """n non-zero integer multipliers, |y| <= 8."""
    return (rng.integers(1, 9, n) * _side(rng, n)).astype(np.float64)


def _put_viol(rng, k, rows, steps, side=None):
    side = _side(rng, len(rows)) if side is None else side
    k[rows] = side * (BAND + np.asarray(steps))


def columns(M, seed=0, amax=128):
    """v[M][24], y[M][24] and one name per column: one slot per scenario of the selection (module docstring of
    tests/test_gpu_select.py says which branch each is for).  Where M is too small for a count, what fits.
    amax: the three `ns` columns carry amax - 1, amax and amax + 1 multipliers."""
    rng = np.random.default_rng([seed, M, amax])
    ks, ys, names = [], [], []

    def col(name, fill):
        k, y = _inside(rng, M), np.zeros(M)
        fill(k, y)
        assert np.abs(k).max(initial=0) <= KMAX
        ks.append(k); ys.append(y); names.append(name)

    pick = lambda n, among=None: rng.choice(M if among is None else among, min(n, M if among is None else len(among)),
                                            replace=False)
    free = lambda y, k=None: np.flatnonzero((y == 0) & (np.abs(k) <= BAND if k is not None else True))

    col("nothing", lambda k, y: None)

    def distinct(k, y):                  # (the grid holds KMAX - BAND = 191 different violations: "200" is what fits)
        rows = pick(KMAX - BAND)
        _put_viol(rng, k, rows, rng.permutation(KMAX - BAND)[:len(rows)] + 1)
    col("distinct", distinct)

    col("all_tie", lambda k, y: _put_viol(rng, k, pick(300), 7))

    def tie_lanes(k, y):
        _put_viol(rng, k, pick(50), rng.integers(1, 9, min(50, M)))
        top = np.array([r for r in (5, 6, 69, 261, 5 + 256 * 17, M - 1) if 0 <= r < M])
        _put_viol(rng, k, top, 100)
    col("tie_lanes", tie_lanes)

    for nvw in (256, 257):
        col(f"nv{nvw}", lambda k, y, nvw=nvw: _put_viol(rng, k, pick(nvw), rng.integers(1, 6, min(nvw, M))))

    for ns in (amax - 1, amax, amax + 1):
        def many(k, y, ns=ns):
            rows = pick(ns)
            y[rows] = _mult(rng, len(rows))
            k[rows] = rng.integers(-BAND - 20, BAND + 21, len(rows))
            oth = pick(40, free(y))
            _put_viol(rng, k, oth, rng.integers(1, 30, len(oth)))
        col(f"ns{ns}", many)

    def mult_on_violated(k, y):
        rows = pick(20)
        y[rows] = _mult(rng, len(rows))
        _put_viol(rng, k, rows, 50)                                   # (side drawn independently of the sign of y)
        oth = pick(30, free(y))
        _put_viol(rng, k, oth, rng.integers(40, 61, len(oth)))        # some above, some below, some AT 50 steps
    col("mult_on_violated", mult_on_violated)

    def up_down_pairs(k, y):
        rows = pick(120)
        rows = rows[:len(rows) // 2 * 2]
        d = rng.integers(1, 12, len(rows) // 2)
        _put_viol(rng, k, rows[0::2], d, side=np.ones(len(d), np.int64))
        _put_viol(rng, k, rows[1::2], d, side=-np.ones(len(d), np.int64))
    col("up_down_pairs", up_down_pairs)

    def one_thread(k, y):
        oth = pick(100, np.flatnonzero(np.arange(M) % 256 != 5))
        _put_viol(rng, k, oth, rng.integers(1, 21, len(oth)))
        own = np.arange(5, M, 256)
        _put_viol(rng, k, own, 150 - rng.integers(0, 3, len(own)))    # three tied levels, all above the others
    col("one_thread", one_thread)

    def ends(k, y):
        oth = pick(30)
        _put_viol(rng, k, oth, rng.integers(1, 50, len(oth)))
        _put_viol(rng, k, np.unique([0, M - 1]), 120)
    col("ends", ends)

    def neg_zero(k, y):
        rows = pick(25)
        _put_viol(rng, k, rows, rng.integers(1, 10, len(rows)))
        y[rows] = -0.0
        oth = pick(3, np.setdiff1d(np.arange(M), rows))
        y[oth] = _mult(rng, len(oth))
    col("neg_zero", neg_zero)

    def all_violated(k, y):              # (nv = M: scanned, never collected -- and there too one thread owns the winners)
        _put_viol(rng, k, np.arange(M), rng.integers(1, 101, M))
        own = np.arange(7, M, 256)
        _put_viol(rng, k, own, 103 - rng.integers(0, 3, len(own)))
    col("all_violated", all_violated)

    def few_mult_no_viol(k, y):
        rows = pick(5)
        y[rows] = _mult(rng, len(rows))
    col("few_mult_no_viol", few_mult_no_viol)

    for i, ns in enumerate((0, 3, 60, 100, 125, 8, 1, 128)):
        def rand(k, y, ns=ns):
            k[:] = rng.integers(-BAND - 6, BAND + 7, M)                 # a band slightly wider than [vlo, vhi]
            rows = pick(ns)
            y[rows] = _mult(rng, len(rows))
        col(f"random{i}_ns{ns}", rand)

    assert len(names) == T
    v = np.ascontiguousarray(np.stack(ks, axis=1) * G)
    return v, np.ascontiguousarray(np.stack(ys, axis=1)), names


def node_terms(v, seed=0):
    """pnq double[3][M][T] around v: pnq[0] = v (the tree forms on star_forest(M) turn it into itself), free counts 1,
    pnq[2] = minus small integers times g."""
    rng = np.random.default_rng([seed, 77])
    return np.ascontiguousarray(np.stack([v, np.ones_like(v), -rng.integers(0, 40, v.shape) * G]))


def restate(v, y, pnq, vlo, vhi, kadd, amax=128):
    """What a rows kernel and the selection behind it leave for multipliers y[m][T] and row voltages v[m][T]:
    vfull, viol (0 where y != 0), sums double[T][4] = {largest row residual, D, rows with y != 0, violated rows with
    y = 0}, cidx int64[T][amax], ccnt int32[T] (-1: more multipliers than amax), cval double[T][3][amax] = sign |
    gradient | multiplier, padding (ci = 0, cs = 1, cg = 0, cy = 0) included.  The list: rows with y != 0 in row order,
    then the min(kadd, amax - ns) most violated rows without one, larger violation first, ties to the lower row."""
    v, y = np.asarray(v, np.float64), np.asarray(y, np.float64)
    m, nt = v.shape
    has = y != 0
    up = (y > 0) | (~has & (v > vhi))
    bound = np.where(up, vhi, vlo)
    over = np.maximum(np.maximum(v - vhi, vlo - v), 0.0)
    viol = np.where(has, 0.0, over)
    sums = np.stack([np.where(has, np.abs(v - bound), over).max(axis=0),
                     (np.asarray(pnq)[2] - np.maximum(vhi * y, vlo * y)).sum(axis=0),
                     has.sum(axis=0).astype(np.float64), (viol > 0).sum(axis=0).astype(np.float64)], axis=1)
    cidx, ccnt = np.zeros((nt, amax), np.int64), np.zeros(nt, np.int32)
    cval = np.zeros((nt, 3, amax))
    cval[:, 0] = 1.0
    rows = np.arange(m)
    for t in range(nt):
        ns, nv = int(sums[t, 2]), int(sums[t, 3])
        if ns > amax:
            ccnt[t] = -1
            continue
        ranked = np.lexsort((rows, -viol[:, t]))[:nv]
        lst = np.concatenate([rows[has[:, t]], ranked[:max(min(kadd, amax - ns), 0)]])
        n = len(lst)
        ccnt[t] = n
        cidx[t, :n] = lst
        cval[t, 0, :n] = np.where(up[lst, t], 1.0, -1.0)
        cval[t, 1, :n] = v[lst, t] - bound[lst, t]
        cval[t, 2, :n] = np.where(has[lst, t], y[lst, t], 0.0)
    return dict(vfull=v.copy(), viol=viol, sums=sums, cidx=cidx, ccnt=ccnt, cval=cval)


def star_forest(M):
    """(parent, edge_r, cons_of) of M nodes that each hang off the substation by an edge of resistance 0.5: through
    revs_admm_amd.feeder.feeder_tree (w = 2 r = 1) the tree form of R p is p itself."""
    return np.full(M, -1, np.int64), np.full(M, 0.5), np.arange(M, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(M, amax=128):
    """columns(M) and their node terms, computed once per size and shared by the tests (read-only)."""
    v, y, names = columns(M, 0, amax)
    pnq = node_terms(v)
    for a in (v, y, pnq):
        a.setflags(write=False)
    return v, y, pnq, names


@functools.lru_cache(maxsize=None)
def expected(M, kadd, amax=128):
    v, y, pnq, _ = case(M, amax)
    out = restate(v, y, pnq, VLO, VHI, kadd, amax)
    for a in out.values():
        a.setflags(write=False)
    return out
