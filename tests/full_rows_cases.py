"""What the full-rows PDHG tests (tests/test_full_rows_cases.py on the host, tests/test_gpu_full_rows.py on the GPU) share:
the atlas of tests/window_cases.py per horizon, its zero and mid-run state, and the classification of its residences by
how many passes ro.home_solve_relaxed_pdhg(dtype=float32, full_rows=True) -- the kernel's step-for-step restatement --
needs with the kernel's tolerance and check interval.

The kernel stops a residence at revs_pdhg_t::max_iter = 4000 passes.  A residence the restatement settles in fewer than
SURE = 3000 passes is one the kernel must settle too; one the restatement has not settled after CAP = 5000 is one the
kernel must flag (status bit 1); in between, float rounding decides on which side of 4000 a residence falls, and no test
asks.  The share of residences that are not settled before SURE is capped by the host test."""
import numpy as np

import window_cases as wc

TOL, CHECK, CAP, SURE = 1e-6, 4, 5000, 3000      # revs_pdhg_t: tol (automatic, full rows), check; the restatement's cap
BAR = 2e-4 * 7.2                                 # kW: tests/test_gpu_agent.py::test_pdhg_full_rows_matches_oracle
_CASES, _CLASSES = {}, {}


def case(T):
    """-> (atlas, workload, oracle homes) of horizon T, built once."""
    from helpers import oracle_homes
    if T not in _CASES:
        a = wc.atlas_of(T)
        w = wc.workload(a)
        _CASES[T] = (a, w, oracle_homes(w))
    return _CASES[T]


def start(w, T, zero):
    """(P_est[k], P_est[k+1], P_sch, G): the zero state (lpsolver.py:244-246) or tests/param_cases.py's mid-run state."""
    from param_cases import state
    n = len(w.homes)
    return (np.zeros((n, T)),) * 4 if zero else state(w, T)


def generator_case(T):
    """-> (workload, oracle homes, mid-run state, ro.home_solve_relaxed's answer, the restatement's passes) of 300
    residences with revs_admm_amd.synthetic.make_workload's windows at horizon T, once.  Seed and state are those of
    tests/test_gpu_shapes.py::test_one_iteration_relaxed_at_band_edges.  (The draw matters to the GPU test that asks for
    a clean status everywhere: a window of a hundred slots that ends with the horizon can need more than the kernel's
    4000 passes at a 1e-6 step -- other draws at T = 128 and 191 hold one to four such residences -- which is PDHG's
    rate on a long triangle and not the step bound: no row lies behind such a window.  The host test holds this draw
    to fewer than SURE passes.)"""
    from oracle import revs_oracle as ro
    from param_cases import state
    from test_gpu_agent import _prep
    key = ("generator", T)
    if key not in _CASES:
        w, oh = _prep(300, T, seed=100 + T, binary_feasible=False)
        st = state(w, T + 1)
        ref = ro.home_solve_relaxed(w.cost, oh, st[0], st[2], st[3], w.kappa)
        n_it = ro.home_solve_relaxed_pdhg(w.cost, oh, st[0], st[2], st[3], w.kappa, iters=CAP, tol=TOL, check=CHECK,
                                          dtype=np.float32, full_rows=True)[3]
        _CASES[key] = (w, oh, st, ref, n_it)
    return _CASES[key]


def classify(T, zero):
    """-> dict: passes (n,) of the float32 restatement from a cold start (CAP where it did not settle), p its schedule,
    ref = ro.home_solve_relaxed's (p, soc, g, status); sure / capped / between: (n,) bool over the feasible EV
    residences.  Once per (T, state)."""
    from oracle import revs_oracle as ro
    key = (T, bool(zero))
    if key not in _CLASSES:
        a, w, oh = case(T)
        pe_old, _, ps, gm = start(w, T, zero)
        ref = ro.home_solve_relaxed(w.cost, oh, pe_old, ps, gm, w.kappa)
        p, _, _, n_it, _ = ro.home_solve_relaxed_pdhg(w.cost, oh, pe_old, ps, gm, w.kappa, iters=CAP, tol=TOL, check=CHECK,
                                                      dtype=np.float32, full_rows=True)
        ok = oh.ev & (ref[3] == 0)
        _CLASSES[key] = dict(passes=n_it, p=p, ref=ref, feasible=ok, sure=ok & (n_it < SURE), capped=ok & (n_it >= CAP),
                             between=ok & (n_it >= SURE) & (n_it < CAP))
    return _CLASSES[key]
