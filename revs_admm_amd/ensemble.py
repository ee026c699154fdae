"""S scenarios of one feeder as ONE ADMM run.

The scenarios of a study share the residences and their nodes; only the EV records (and possibly the loads) differ.
Their state is kept as float[n][S][T] and read two ways, without a copy:

  the operator's view    n residences x (S T) columns.  The operator's slots are independent problems that share R
                         (revs_admm_ops.h), so this is the dual Newton path as it is, with T' = S T columns.
  the residences' view   n S residences x T slots, one 32-byte record per (residence, scenario): the sweep
                         (revs_agent_step_out), the residuals and the status reduction as they are, with n' = n S.

`AdmmEngine` names both shapes: (n, T) for the state arrays and everything node-side, (sweep_n, sweep_T) for the calls
that pass residence-side buffers (engine.py, _init_residences).  `AdmmEnsemble` is an `AdmmEngine` with (n, T) = (n, S T)
and a sweep shape of (n S, T): all it adds to the construction is how records and load are laid out for the sweep.  Its
options keep `step()` on the general branch -- `operator_solve()` then `agent_step()` -- because the steady-state and
chained launches carry one T for both sides.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib
from ._lib import HOME_DTYPE
from .engine import AdmmEngine, OperatorOptions, _on_current_stream
from .ensemble_bills import EnsembleBillsMixin
from .ensemble_certificate import EnsembleCertificateMixin
from .ensemble_convergence import EnsembleConvergenceMixin
from .ensemble_report import EnsembleReportMixin

# the ADMM forms of the operator QP (operator_admm.py) multiply by the dense factors of R: the dense products' column limit
ADMM_FORM_MAX_COLS = _lib.MAX_T


def check_shape(S: int, T: int, group=None) -> None:
    """The limits of an ensemble, checked before anything touches the device."""
    if group is not None:
        raise NotImplementedError("AdmmEnsemble: ensembles run on one GPU (residences sharded over a process group: "
                                  "one AdmmEngine per scenario)")
    if S < 1:
        raise ValueError("AdmmEnsemble: homes_list is empty")
    if not 1 <= T <= _lib.MAX_T:
        raise ValueError(f"AdmmEnsemble: T = {T} outside 1..{_lib.MAX_T}")
    if S * T > _lib.ENS_MAX_COLS:
        raise ValueError(f"AdmmEnsemble: {S} scenarios x {T} slots = {S * T} columns; one ensemble holds "
                         f"{_lib.ENS_MAX_COLS} (at most {_lib.ENS_MAX_COLS // T} scenarios at T = {T})")


class AdmmEnsemble(EnsembleCertificateMixin, EnsembleReportMixin, EnsembleBillsMixin, EnsembleConvergenceMixin,
                   AdmmEngine):
    """S ADMM runs on one feeder, side by side on one GPU.

    Parameters as AdmmEngine's, except
    homes_list   S arrays of HOME_DTYPE records over the same n residences (scenario s: homes_list[s])
    load         (n, T) shared by the scenarios, or (S, n, T)

    Every scenario's iterates equal those of its own AdmmEngine to the operator's tolerance, not bit for bit: the
    Newton loop's run-wide decisions (rows admitted per iteration, small against general model, stopping once every
    column is within tolerance) look across all scenarios' columns.  Identical scenarios get identical bits.
    """

    def __init__(self, cost, homes_list, load, node_of, Rn, kappa=5.0, vset=1.0, vlow=0.95, vhigh=1.05, mode="binary",
                 device="cuda:0", pdhg=None, op: OperatorOptions | None = None, group=None, pdhg_warm=True, feeder=None,
                 _kernels=None):
        homes_list = [np.asarray(h) for h in homes_list]
        cost = np.asarray(cost, np.float64)
        self.S_count, self.T_slot = len(homes_list), int(cost.shape[0])
        check_shape(self.S_count, self.T_slot, group)
        self.n_res = len(homes_list[0])
        if any(h.dtype != HOME_DTYPE or h.shape != (self.n_res,) for h in homes_list):
            raise ValueError("AdmmEnsemble: every scenario needs one HOME_DTYPE record per residence, the same residences in each")
        load = np.asarray(load, np.float32)
        if load.shape == (self.n_res, self.T_slot):
            load = np.broadcast_to(load[:, None, :], (self.n_res, self.S_count, self.T_slot))
        elif load.shape == (self.S_count, self.n_res, self.T_slot):
            load = load.transpose(1, 0, 2)
        else:
            raise ValueError(f"AdmmEnsemble: load has shape {load.shape}; expected (n, T) = {(self.n_res, self.T_slot)} "
                             f"or (S, n, T) = {(self.S_count, self.n_res, self.T_slot)}")
        o = op or OperatorOptions()
        if o.solver != "newton":
            raise ValueError('AdmmEnsemble: the columns of an ensemble are solved by the dual Newton path (solver="newton")')
        # the general branch of step(): the speculative, chained and streaming launches carry one T for both views
        # (... and the Newton solve as the plan's native call: the Python loop's evaluations may take the dense products)
        o = dataclasses.replace(o, speculate=False, chain=False, fuse_home_pass=False, stream_block=1, preallocate=False,
                                native_plan=True, native_newton=True)
        # (the load goes in as the operator sees it, (n, S T): its shape is the engine's (n, T))
        super().__init__(cost, homes_list, load.reshape(self.n_res, -1), node_of, Rn, kappa=kappa, vset=vset, vlow=vlow,
                         vhigh=vhigh, mode=mode, device=device, pdhg=pdhg, op=o, pdhg_warm=pdhg_warm, feeder=feeder,
                         _kernels=_kernels)
        if self._tree is None and self.T > _lib.MAX_T and _kernels is None:
            raise ValueError(f"AdmmEnsemble: {self.T} columns need the feeder as a tree (feeder=): the dense products "
                             f"R p and R^T y hold {_lib.MAX_T} columns")

    # ---------------------------------------------------------------- the two views
    def _by_scenario(self, t, width):
        """A state tensor as (n, S, width)."""
        return t.view(self.n_res, self.S_count, width)

    # ---------------------------------------------------------------- construction stages
    def _init_problem(self, homes_list, *args):
        # (records without an EV everywhere: the residences are sorted by node only -- the scenarios disagree on who owns one)
        return super()._init_problem(np.zeros(self.n_res, HOME_DTYPE), *args)

    def _sweep_layout(self, homes_list, load):
        """Records [n][S] and load (n S, T): one sweep row per (residence, scenario)."""
        return np.stack(homes_list, axis=1)[self.perm].reshape(-1), load[self.perm].reshape(-1, self.T_slot)

    # ---------------------------------------------------------------- operator side
    def _column_name(self, col):
        return f"scenario {col // self.T_slot}, slot {col % self.T_slot} (column {col})"

    def _worst_column(self):
        """The column whose rows are farthest from their bounds in the last evaluations' stats."""
        st = np.maximum(self.stats_host[0].numpy()[:, 0], self.stats_host[1].numpy()[:, 0])
        return int(np.argmax(np.nan_to_num(st, nan=np.inf)))

    def _ensure_admm(self):
        if self.T > ADMM_FORM_MAX_COLS:
            raise _lib.RevsError(
                f"REVS_ENOTCONV: the dual Newton path could not finish an ensemble of {self.T} columns -- worst rows in "
                f"{self._column_name(self._worst_column())} -- and the ADMM forms of the operator QP hold "
                f"{ADMM_FORM_MAX_COLS} columns: solve that scenario on its own engine, or in ensembles of at most "
                f"{ADMM_FORM_MAX_COLS // self.T_slot} scenarios")
        super()._ensure_admm()

    def _ensure_big(self):
        if self.T > _lib.MAX_T:      # (its evaluations go through the dense products)
            return None
        try:
            return super()._ensure_big()
        except torch.cuda.OutOfMemoryError:      # (the lists of 512 rows grow with the columns: ~13 GB at 1024)
            self._big = None
            return None

    def _operator_solve_newton_big(self, newton0=0, evals0=0, pivots0=0):
        if self._ensure_big() is None:
            # no room for (or no dense product behind) the lists of up to 512 rows: the iteration goes to the ADMM forms
            self.yd[0].zero_()
            return self._solve_book(False, newton0, evals0, pivots0, 0, 0, None, arm=False)
        return super()._operator_solve_newton_big(newton0, evals0, pivots0)

    def multipliers(self, s):
        """The voltage rows' multipliers of scenario s, (M, T)."""
        return self.yd[0].view(self.M, self.S_count, self.T_slot)[:, s, :].cpu().numpy()

    # ---------------------------------------------------------------- residence side
    def scenario_max_diff(self):
        """max_h diff[h] of the iteration just finished, per scenario (S,)."""
        return self.diff.view(self.n_res, self.S_count).amax(0).cpu().numpy().astype(np.float64)

    def run_steps(self, count):
        for _ in range(count):
            self.step(write_sc=False)

    @_on_current_stream
    def run(self, iter_max=15, eps=None, history=True):
        """solve_ADMM's loop for every scenario -> diff (S, iterations, n) in the caller's residence order.  With `eps`
        the run stops after the first iteration in which every scenario's max_h diff[h] is within it (schedules are
        then written by every iteration).  history="device": the history is not fetched -- it stays on the device as
        `self.diff_history`, (iterations, n S) float32 in the sweep's layout, for convergence_report(); returns the
        number of iterations run."""
        n, S = self.n_res, self.S_count
        on_device = self._history_on_device(history, iter_max)
        hist = torch.empty((iter_max, n * S), dtype=torch.float32, device=self.dev)
        k = 0
        while k < iter_max:
            self.step(write_sc=eps is not None or k == iter_max - 1)
            hist[k].copy_(self.diff)
            k += 1
            if k == 1:
                self.check_status()          # a residence without a solution is reported after the first iteration
            if eps is not None and (self.scenario_max_diff() <= eps).all():
                break
        self.check_status()
        if on_device:
            self.diff_history = hist[:k]
            return k
        d = hist[:k].view(k, n, S).permute(2, 0, 1).cpu().numpy()
        return np.ascontiguousarray(d[:, :, self.inv_perm])

    def _rule_shape(self):
        """rule_schedule()'s net load as the reports' profile= takes it: (n, S, T)."""
        return (self.n_res, self.S_count, self.T_slot)

    # ---------------------------------------------------------------- state in / out
    def set_state(self, s, P_est, P_sch, G, iteration=None):
        """Load (P_est[k], P_sch[k], G[k]) of scenario s in the caller's residence order; the operator's multipliers stay
        as a warm start."""
        for t, a in ((self.P_est, P_est), (self.P_sch, P_sch), (self.G, G)):
            a = np.ascontiguousarray(np.asarray(a, np.float32)[self.perm])
            assert a.shape == (self.n_res, self.T_slot)
            self._by_scenario(t, self.T_slot)[:, s, :].copy_(torch.from_numpy(a))
        self._sc_iteration = -1
        if iteration is not None:
            self.iteration = int(iteration)

    def get_state(self, s):
        """(P_est[k], P_sch[k], G[k]) of scenario s in the caller's residence order."""
        return tuple(self._by_scenario(t, self.T_slot)[:, s, :].cpu().numpy()[self.inv_perm]
                     for t in (self.P_est, self.P_sch, self.G))

    def _zero_state(self):
        """AdmmEngine.reset()'s step into the state: every scenario back to iteration 0 (the rest of reset() -- multipliers,
        books, flags -- is the parent's, in the operator's view)."""
        for t in (self.P_est, self.P_sch, self.G):
            t.zero_()
        self.iteration = 0
        self._sc_iteration = -1

    def result(self):
        """(P_sch, S, C) of the last iteration, each with a leading scenario axis, in the caller's residence order."""
        T = self.T_slot
        out = tuple(np.ascontiguousarray(self._by_scenario(t, w).permute(1, 0, 2).cpu().numpy()[:, self.inv_perm])
                    for t, w in ((self.P_sch, T), (self.S, T), (self.Csoc, T + 1)))
        self.check_status()
        return out

    def _one_schedule_only(self, *a, **k):
        raise NotImplementedError("AdmmEnsemble: this method takes one schedule -- every scenario's bound and certificate "
                                  "come from lower_bounds() / certificates(), every scenario's report from study_report() / "
                                  "network_reports() (node_sums() for the sums alone), every scenario's voltages from "
                                  "voltages()")

    network_report = lower_bound = certificate = voltage = _one_schedule_only
