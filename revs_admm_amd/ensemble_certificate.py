"""Certificates of an ensemble: every scenario's dual bound in one launch (revs_dual_bound_many, DESIGN.md sections 3.6
and 3.9).  What certificate.py does for one run, for the S scenarios of an AdmmEnsemble at once and on the ensemble's
own layout -- the records [n][S], node arrays double[M][S T] with scenario s in columns s T + t -- so nothing is copied
per scenario: one node sum of the schedules, one R y over all S T columns, and per evaluation of the line search one
launch and one read-back for all scenarios (certificate.ray_search_many).  The kernel gives every scenario the bits
revs_dual_bound gives on that scenario alone.  Methods of AdmmEnsemble (mixed in by ensemble.py); nothing here touches
the run's state."""
from __future__ import annotations

import ctypes as C
import math
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .certificate import Certificate, ray_search_many

# columns of one dense f64 product (revs_gemm_tn_f64)
DENSE_MAX_COLS = _lib.MAX_T


class EnsembleCertificateMixin:
    _bdm = None

    def _bounds_setup(self):
        """Buffers of the batched bound, once per ensemble: node_of in the engine's order (shared by the scenarios),
        the node sums of every scenario's LOAD (M, S T), scratch, one scale and one result row per scenario."""
        if self._bdm is not None:
            return self._bdm
        lib, M, S, T, n = self.lib, self.M, self.S_count, self.T_slot, self.n_res
        f64 = dict(dtype=torch.float64, device=self.dev)
        bd = SimpleNamespace()
        counts = np.diff(self.node_ptr.cpu().numpy())
        bd.node_of = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), counts)).to(self.dev)
        bd.scratch = torch.zeros(max(1, int(lib.revs_dual_bound_many_scratch(n, S, T))), **f64)
        bd.out = torch.zeros(S, 4, **f64)
        bd.scale = torch.zeros(S, **f64)
        bd.lsum = torch.zeros(M, S * T, **f64)
        if n:
            ld = self.load.double()          # (n S, T) = (n, S T): the operator's view
            check(lib.revs_aggregate_f64(M, S * T, ptr(self.node_ptr), ptr(ld), None, ptr(bd.lsum), self.stream),
                  "revs_aggregate_f64")
            del ld
        bd.has = torch.from_numpy((np.asarray(self.node_counts) > 0).astype(np.float64)).to(self.dev)[:, None]
        self._bdm = bd
        return bd

    def _bounds_dense_R(self, x, out):
        """out = R x over all S T columns by the dense f64 product, which holds DENSE_MAX_COLS columns: past that,
        column slices of whole scenarios (the entry takes leading dimensions)."""
        M, S, T = self.M, self.S_count, self.T_slot
        per = S if S * T <= DENSE_MAX_COLS else max(1, DENSE_MAX_COLS // T)
        for a in range(0, S, per):
            b = min(S, a + per)
            check(self.lib.revs_gemm_tn_f64(M, (b - a) * T, M, ptr(self.R64), M, x.data_ptr() + 8 * a * T, S * T,
                                            out.data_ptr() + 8 * a * T, S * T, 0, self.stream), "revs_gemm_tn_f64")
        return out

    def _bounds_R(self, x, out):
        """out = R x (double[M][S T]) at the rows with residences: the tree form where the engine holds the feeder."""
        if self._tree is None:
            return self._bounds_dense_R(x, out)
        out.zero_()                     # (the tree writes the rows with residences only)
        check(self.lib.revs_tree_voltage(self.M, self.T, C.byref(self._tree), ptr(x), self.vlo, self.vhi, ptr(out),
                                         None, self.stream), "revs_tree_voltage")
        return out

    def _bounds_launch(self, n_res, d, y, load_node, scale, integral):
        """One revs_dual_bound_many and its read-back -> (S, 4) on the host."""
        bd = self._bdm
        bd.scale.copy_(torch.from_numpy(np.ascontiguousarray(scale, np.float64)))
        check(self.lib.revs_dual_bound_many(n_res, self.S_count, self.T_slot, ptr(self.cost),
                                            ptr(self.homes) if n_res else None, ptr(bd.node_of) if n_res else None,
                                            self.M, ptr(d), ptr(y), ptr(load_node), ptr(bd.scale), self.vlo, self.vhi,
                                            int(integral), ptr(bd.scratch), ptr(bd.out), self.stream),
              "revs_dual_bound_many")
        return bd.out.cpu().numpy()

    def _bounds_eval(self, d, y, scale, integral):
        """L_s(scale[s] y_s) of every scenario: (values (S,), empty residences (S,)) -- +inf where a residence's own rows
        are empty."""
        h = self._bounds_launch(self.n_res, d, y, self._bdm.lsum, scale, integral)
        empties = h[:, 3].astype(np.int64)
        return np.where(empties > 0, math.inf, (h[:, 0] + h[:, 1]) + h[:, 2]), empties

    def _bounds_dot_c(self, x):
        """sum_{n,t} c_t x[n][s T + t] per scenario, in f64 (the batched bound with no residences and no multipliers:
        its LOAD term)."""
        return self._bounds_launch(0, None, None, x, np.zeros(self.S_count), False)[:, 1].copy()

    def _bounds_scales(self, scale):
        s = np.asarray(scale, np.float64)
        if s.ndim == 0:
            s = np.full(self.S_count, float(s))
        if s.shape != (self.S_count,):
            raise ValueError(f"scale: a scalar or {(self.S_count,)} values, not shape {s.shape}")
        if not (s >= 0).all():       # (also rejects NaN; the kernel reads the scales on the device and cannot refuse one)
            raise ValueError("scale must be >= 0")
        return s

    def _bounds_multipliers(self, multipliers):
        """(M, S T) multipliers in the operator's view, rows without residences dropped."""
        bd, M, S, T = self._bdm, self.M, self.S_count, self.T_slot
        if isinstance(multipliers, str):
            if multipliers != "operator":
                raise ValueError(f"multipliers: 'operator' or an (S, M, T) array, not {multipliers!r}")
            use = self.op.solver == "newton" and self._y_support
            y = self.yd[0].clone() if use else torch.zeros_like(bd.lsum)
        else:
            y = np.asarray(multipliers, np.float64)
            if y.shape != (S, M, T):
                raise ValueError(f"multipliers: shape {y.shape}, expected {(S, M, T)}")
            y = torch.from_numpy(np.ascontiguousarray(y.transpose(1, 0, 2)).reshape(M, S * T)).to(self.dev)
        return (y * bd.has).contiguous()

    def _bounds_integral(self, integral):
        return self.mode == _lib.MODE_BINARY if integral is None else bool(integral)

    def lower_bounds(self, y=None, scale=1.0, integral=None):
        """AdmmEngine.lower_bound for every scenario in one evaluation -> (S,) float64: L_s(scale[s] y_s) <= optimum of
        scenario s's centralized problem.  y: (S, M, T) signed row multipliers, default the operator's current ones
        (zero when its last solve left no support); scale: a scalar or (S,) values, each >= 0; integral: as there.
        +inf for a scenario with a residence whose own rows are empty."""
        scale = self._bounds_scales(scale)
        self._bounds_setup()
        yv = self._bounds_multipliers("operator" if y is None else y)
        d = self._bounds_R(yv, torch.empty_like(yv))
        return self._bounds_eval(d, yv, scale, self._bounds_integral(integral))[0]

    def certificates(self, multipliers="operator", search=True) -> list:
        """AdmmEngine.certificate for every scenario -> S Certificates (see there).  multipliers: "operator" or an
        (S, M, T) array; search: maximise every L_s(s y_s) over s >= 0 in lock-step -- one batched evaluation serves a
        step of every scenario's own search (certificate.ray_search_many), so `evaluations` (shared by the S
        certificates, as `seconds`, the wall time of this call) is the longest scenario's count, not the sum --
        otherwise s = 1; a scenario whose multipliers are all zero takes s = 0.  No supergradient ascent (DESIGN.md
        section 7): ascent_steps = 0.  The run's state (schedules, multipliers, buffers) is not touched."""
        t_start = time.perf_counter()
        bd = self._bounds_setup()
        lib, M, S, T = self.lib, self.M, self.S_count, self.T_slot
        integral = self._bounds_integral(None)
        # ---- the schedules: cost and worst row against EVERY row, per scenario ----
        gsum = torch.zeros(M, S * T, dtype=torch.float64, device=self.dev)
        if self.n_res:
            g = self.P_sch.double()
            check(lib.revs_aggregate_f64(M, S * T, ptr(self.node_ptr), ptr(g), None, ptr(gsum), self.stream),
                  "revs_aggregate_f64")
            del g
        upper = self._bounds_dot_c(gsum)
        c_load = self._bounds_dot_c(bd.lsum)
        v = self._bounds_dense_R(gsum, torch.empty_like(gsum)).view(M, S, T)
        over = torch.maximum((v - self.vhi).amax(dim=(0, 2)), (self.vlo - v).amax(dim=(0, 2)))
        max_violation = np.maximum(0.0, over.cpu().numpy())
        del gsum, v
        # ---- the scales along the multipliers ----
        y = self._bounds_multipliers(multipliers)
        d = self._bounds_R(y, torch.empty_like(y))
        zero = ~(y.view(M, S, T) != 0).any(dim=2).any(dim=0).cpu().numpy()
        if search:
            scale, lower, empty, evaluations = ray_search_many(lambda x: self._bounds_eval(d, y, x, integral), S,
                                                               skip=zero)
        else:
            scale = np.where(zero, 0.0, 1.0)
            lower, empty = self._bounds_eval(d, y, scale, integral)
            evaluations = 1
        seconds = time.perf_counter() - t_start
        out = []
        for s in range(S):
            lo, up = float(lower[s]), float(upper[s])
            gap = (up - lo) / abs(lo) if lo not in (0.0, math.inf) else math.inf
            charge = lo - float(c_load[s])
            gap_ev = (up - lo) / abs(charge) if charge != 0.0 and not math.isinf(lo) else math.inf
            mv = float(max_violation[s])
            out.append(Certificate(lower=lo, upper=up, gap=gap, gap_ev=gap_ev, max_violation=mv,
                                   feasible=mv <= self.op.eps * self._scale, scale=float(scale[s]), ascent_steps=0,
                                   evaluations=int(evaluations), seconds=seconds, empty=int(empty[s]),
                                   integral=integral))
        return out
