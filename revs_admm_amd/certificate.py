"""How far a schedule is from the best possible one: the comparison of the reference's test-centralopt.py:98-116
(distributed schedule against a centralized solve) at sizes no LP solver holds.  The centralized problem is
oracle.solve_central_lp's (min sum_h c.g_h over every residence's own rows and every voltage row); its optimum is
bracketed by
  * upper = sum c.P_sch of the current schedules -- an upper bound wherever P_sch satisfies the rows (max_violation);
  * lower = L(lambda), the Lagrangian dual bound of the rows at multipliers lambda = s y (revs_dual_bound: one pass
    over the 32-byte residence records), which no choice of lambda can push above the optimum.
The multipliers come from the operator's QP (its dual Newton solution y; at the ADMM's fixed point the residences
solve exactly L's subproblem at s = 1), the scale by a search along the ray, and optionally a
few supergradient steps.  Methods of AdmmEngine (mixed in by engine.py); nothing here touches the run's state."""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def _ray_search_steps():
    """The search of certificate(search=True) along a ray, written once as a generator: it yields every scale it wants
    evaluated (each distinct scale once: the memo is here), is sent (value, empty) for it, and returns
    (s, value, empty) of the best scale seen -- ties to the smaller scale.  L(s y) is concave in s >= 0: the value at 0
    and 1, doubling while the value rises, then 24 golden-section steps on the bracket."""
    seen = {}

    def phi(x):
        if x not in seen:
            seen[x] = yield x
        return seen[x][0]
    f0, f1 = (yield from phi(0.0)), (yield from phi(1.0))
    if math.isinf(f0):
        a = b = 0.0
    elif f1 <= f0:
        a, b = 0.0, 1.0
    else:
        x = 1.0
        for _ in range(60):
            if (yield from phi(2.0 * x)) <= (yield from phi(x)):
                break
            x *= 2.0
        a, b = (x / 2.0 if x > 1.0 else 0.0), 2.0 * x
    if b > a:
        x1, x2 = b - _GOLD * (b - a), a + _GOLD * (b - a)
        for _ in range(24):
            if (yield from phi(x1)) < (yield from phi(x2)):
                a, x1, x2 = x1, x2, x1 + _GOLD * (b - x1)
            else:
                b, x2, x1 = x2, x1, x2 - _GOLD * (x2 - a)
    s = max(seen, key=lambda k: (seen[k][0], -k))
    return (s, *seen[s])


def ray_search(phi):
    """Maximise a concave phi over s >= 0: phi(x) -> (value, empty) is one evaluation; -> (s, value, empty)."""
    steps = _ray_search_steps()
    try:
        x = next(steps)
        while True:
            x = steps.send(phi(x))
    except StopIteration as done:
        return done.value


def ray_search_many(phi_many, S, skip=None):
    """ray_search for S rays in lock-step: phi_many(scales (S,)) -> (values (S,), empties (S,)) is ONE batched
    evaluation.  Every scenario keeps its own bracket, memo and phase (its own _ray_search_steps), so the distinct
    scales it has evaluated, its chosen s and its value are exactly ray_search's on its phi alone; a scenario with
    nothing new to ask in a round resubmits the last scale it asked for and the answer is ignored.  skip[s]: the
    scenario takes s = 0 (its multipliers are zero: the ray is a point).
    -> (s (S,), values (S,), empties (S,) int, batched evaluations)."""
    skip = np.zeros(S, bool) if skip is None else np.asarray(skip, bool)
    steps = [None if skip[s] else _ray_search_steps() for s in range(S)]
    ask = np.zeros(S)                       # (a skipped scenario asks for 0 once)
    done = [None] * S
    for s, st in enumerate(steps):
        if st is not None:
            ask[s] = next(st)
    rounds = 0
    while any(d is None for d in done):
        values, empties = phi_many(ask.copy())
        rounds += 1
        for s, st in enumerate(steps):
            if done[s] is not None:
                continue
            got = (float(values[s]), int(empties[s]))
            if st is None:
                done[s] = (0.0, *got)
                continue
            try:
                ask[s] = st.send(got)
            except StopIteration as end:
                done[s] = end.value
    return (np.array([d[0] for d in done]), np.array([d[1] for d in done]),
            np.array([d[2] for d in done], np.int64), rounds)


@dataclass
class Certificate:
    """lower <= optimum of the centralized problem (the MILP with on/off chargers, the LP otherwise); upper = the
    schedules' cost.  gap = (upper - lower) / |lower| is a certified optimality gap ONLY when `feasible` holds (the
    schedules satisfy every voltage row to the streaming verdicts' tolerance); gap_ev is the same distance relative to
    the charging part of the bound, lower - c.sum(LOAD)."""
    lower: float
    upper: float
    gap: float
    gap_ev: float
    max_violation: float
    feasible: bool
    scale: float
    ascent_steps: int
    evaluations: int
    seconds: float
    empty: int = 0           # residences whose own rows are empty (the problem is infeasible: lower = +inf)
    integral: bool = False   # the bound of the on/off chargers' MILP


class CertificateMixin:
    _bd = None

    def _bound_setup(self):
        """Buffers of the bound, once per engine: the residences' rows (node_of in the engine's order), the node sums
        of LOAD (this rank's: the LOAD term is additive over ranks), scratch."""
        if self._bd is not None:
            return self._bd
        lib, M, T, n = self.lib, self.M, self.T, self.sweep_n
        f64 = dict(dtype=torch.float64, device=self.dev)
        bd = SimpleNamespace()
        counts = np.diff(self.node_ptr.cpu().numpy())
        bd.node_of = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), counts)).to(self.dev)
        bd.scratch = torch.zeros(max(1, int(lib.revs_dual_bound_scratch(n, self.sweep_T))), **f64)
        bd.out = torch.zeros(4, **f64)
        bd.lsum = torch.zeros(M, T, **f64)
        if n:
            ld = self.load.double()
            check(lib.revs_aggregate_f64(M, T, ptr(self.node_ptr), ptr(ld), None, ptr(bd.lsum), self.stream),
                  "revs_aggregate_f64")
            del ld
        bd.has = torch.from_numpy((np.asarray(self.node_counts) > 0).astype(np.float64)).to(self.dev)[:, None]
        bd.lsum_all = None          # the node sums of every rank's LOAD (first certificate)
        self._bd = bd
        return bd

    def _bound_R(self, x, out):
        """out = R x (double[M][T]) at the rows with residences: the tree form where the engine holds the feeder, the
        dense f64 product otherwise."""
        if self._tree is not None:
            out.zero_()                 # (the tree writes the rows with residences only)
            check(self.lib.revs_tree_voltage(self.M, self.T, C.byref(self._tree), ptr(x), self.vlo, self.vhi,
                                             ptr(out), None, self.stream), "revs_tree_voltage")
        else:
            check(self.lib.revs_gemm_tn_f64(self.M, self.T, self.M, ptr(self.R64), self.M, ptr(x), self.T, ptr(out),
                                            self.T, 0, self.stream), "revs_gemm_tn_f64")
        return out

    def _bound_launch(self, d, y, scale, integral, p_node=None):
        """Enqueue one evaluation of L(scale y) (d = R y) into self._bd.out -- no synchronisation."""
        bd = self._bd
        check(self.lib.revs_dual_bound(self.sweep_n, self.sweep_T, ptr(self.cost), ptr(self.homes), ptr(bd.node_of),
                                       self.M, ptr(d), ptr(y), ptr(bd.lsum), float(scale), self.vlo, self.vhi, int(integral),
                                       ptr(bd.scratch), ptr(p_node), ptr(bd.out), self.stream), "revs_dual_bound")

    def _bound_eval(self, d, y, scale, integral, p_node=None):
        """L(scale y) over every rank: (value, empty residences).  The residences' part, the LOAD part and the count
        are summed over the ranks in one all-reduce; the row part is every rank's own (the same) and added once."""
        self._bound_launch(d, y, scale, integral, p_node)
        bd = self._bd
        if self.group is not None:
            v = bd.out.clone()
            v[2] = 0.0
            self._allreduce(v)
            h = v.cpu().numpy()
            h[2] = float(bd.out[2])
        else:
            h = bd.out.cpu().numpy()
        self._bound_evals = getattr(self, "_bound_evals", 0) + 1
        if h[3] > 0:
            return math.inf, int(h[3])
        return float((h[0] + h[1]) + h[2]), 0

    def _bound_dot_c(self, x):
        """sum_{n,t} c_t x[n][t] in f64 (revs_dual_bound with no residences and no multipliers: its LOAD term)."""
        bd = self._bd
        check(self.lib.revs_dual_bound(0, self.T, ptr(self.cost), None, None, self.M, None, None, ptr(x), 0.0,
                                       self.vlo, self.vhi, 0, ptr(bd.scratch), None, ptr(bd.out), self.stream),
              "revs_dual_bound")
        return float(bd.out[1])

    def _bound_multipliers(self, multipliers):
        bd = self._bd
        if isinstance(multipliers, str):
            if multipliers != "operator":
                raise ValueError(f"multipliers: 'operator' or an (M, T) array, not {multipliers!r}")
            # (the dual Newton path's y; zero where its last solve left no row with a multiplier -- yd[0] then holds
            # nothing the run uses -- and on the ADMM forms' path)
            use = self.op.solver == "newton" and self._y_support
            y = self.yd[0].clone() if use else torch.zeros_like(bd.lsum)
        else:
            y = torch.as_tensor(np.asarray(multipliers, np.float64)).to(self.dev)
            if tuple(y.shape) != (self.M, self.T):
                raise ValueError(f"multipliers: shape {tuple(y.shape)}, expected {(self.M, self.T)}")
        # (rows without residences are dropped: the tree form carries only the others, and fewer rows only relax)
        return (y * bd.has).contiguous()

    def lower_bound(self, y=None, scale=1.0, integral=None):
        """One evaluation of the Lagrangian dual bound L(scale * y) <= optimum of the centralized problem.
        y: (M, T) signed row multipliers (y > 0 at vhi, y < 0 at vlo), default the operator's current ones;
        integral: the on/off chargers' MILP bound (default: the engine's mode -- binary -> MILP, otherwise LP).
        +inf when some residence's own rows are empty (the centralized problem is infeasible)."""
        if scale < 0:
            raise ValueError("scale must be >= 0")
        self._bound_setup()
        integral = self.mode == _lib.MODE_BINARY if integral is None else bool(integral)
        yv = self._bound_multipliers("operator" if y is None else y)
        d = self._bound_R(yv, torch.empty_like(yv))
        return self._bound_eval(d, yv, scale, integral)[0]

    def certificate(self, multipliers="operator", search=True, ascent=0) -> Certificate:
        """Bracket the optimum of the centralized problem around the current schedules (see Certificate).
        multipliers: "operator" (the dual Newton path's current y; zero on the ADMM forms' path) or an (M, T) array;
        search: maximise L(s y) over s >= 0 (concave along the ray: doubling, then golden section -- about 30
        evaluations), otherwise s = 1; ascent = k: k supergradient steps on lambda = s y from there, Polyak step sizes
        towards `upper`, the best lambda seen kept.  Sharded residences: every rank calls it; one small all-reduce per
        evaluation.  The run's state (schedules, multipliers, buffers) is not touched."""
        t_start = time.perf_counter()
        bd = self._bound_setup()
        lib, M, T = self.lib, self.M, self.T
        self._bound_evals = 0
        integral = self.mode == _lib.MODE_BINARY
        if bd.lsum_all is None:
            bd.lsum_all = bd.lsum.clone()
            self._allreduce(bd.lsum_all)
        # ---- the schedules: cost and worst row against EVERY row solve_central_lp constrains ----
        gsum = torch.zeros(M, T, dtype=torch.float64, device=self.dev)
        if self.n:
            g = self.P_sch.double()
            check(lib.revs_aggregate_f64(M, T, ptr(self.node_ptr), ptr(g), None, ptr(gsum), self.stream),
                  "revs_aggregate_f64")
            del g
        self._allreduce(gsum)
        upper = self._bound_dot_c(gsum)
        c_load = self._bound_dot_c(bd.lsum_all)
        v = torch.empty_like(gsum)
        check(lib.revs_gemm_tn_f64(M, T, M, ptr(self.R64), M, ptr(gsum), T, ptr(v), T, 0, self.stream),
              "revs_gemm_tn_f64")
        max_violation = max(0.0, float((v - self.vhi).max()), float((self.vlo - v).max()))
        del gsum, v
        # ---- the scale along the operator's multipliers ----
        y = self._bound_multipliers(multipliers)
        d = self._bound_R(y, torch.empty_like(y))
        empty = 0
        if not bool(torch.any(y != 0)):
            s = 0.0
            best, empty = self._bound_eval(d, y, s, integral)
        elif not search:
            s = 1.0
            best, empty = self._bound_eval(d, y, s, integral)
        else:
            s, best, empty = ray_search(lambda x: self._bound_eval(d, y, x, integral))
        # ---- supergradient ascent on lambda from s y ----
        # Polyak steps theta (upper - L) / |g|^2 along a supergradient g; upper overestimates the optimum (the
        # schedules are not optimal), so a step that does not raise the bound is taken back and theta halved
        steps = 0
        if ascent > 0 and not empty:
            lam = (y * s).contiguous()
            dl = self._bound_R(lam, torch.empty_like(lam))
            pn, pn_try = torch.zeros_like(lam), torch.zeros_like(lam)
            vv, sg = torch.empty_like(lam), None
            cur, _ = self._bound_eval(dl, lam, 1.0, integral, pn)
            best = max(best, cur)
            theta = 1.0
            for _ in range(int(ascent)):
                if sg is None:
                    self._allreduce(pn)
                    self._bound_R(pn + bd.lsum_all, vv)          # voltages of the minimiser (rows with residences)
                    sg = vv - torch.where(lam > 0, self.vhi, torch.where(lam < 0, self.vlo, vv.clamp(self.vlo, self.vhi)))
                    sg *= bd.has
                    nrm2 = float((sg * sg).sum())
                if not nrm2 > 0.0 or not upper > cur:
                    break                                        # (lambda maximises L, or L reached the schedules' cost)
                trial = (lam + (theta * (upper - cur) / nrm2) * sg).contiguous()
                self._bound_R(trial, dl)
                val, _ = self._bound_eval(dl, trial, 1.0, integral, pn_try.zero_())
                steps += 1
                if val > cur:
                    lam, cur, pn, pn_try, sg = trial, val, pn_try, pn, None
                    best = max(best, cur)
                else:
                    theta *= 0.5
        lower = best
        gap = (upper - lower) / abs(lower) if lower not in (0.0, math.inf) else math.inf
        charge = lower - c_load
        gap_ev = (upper - lower) / abs(charge) if charge != 0.0 and not math.isinf(lower) else math.inf
        return Certificate(lower=lower, upper=upper, gap=gap, gap_ev=gap_ev, max_violation=max_violation,
                           feasible=max_violation <= self.op.eps * self._scale, scale=float(s), ascent_steps=steps,
                           evaluations=self._bound_evals, seconds=time.perf_counter() - t_start, empty=empty,
                           integral=integral)
