"""The convergence report: the statistics of the residual history diff[k][i] -- what the reference's solve_ADMM returns
besides the schedules (lpsolver.py:280-290) and plot_convergence draws (test-dist-ind-opt.py:109-120) -- for one run or
the S scenarios of an ensemble, on the GPU where the streaming launches leave the history (revs_conv_report,
include/revs_admm_ops.h): a box-plot record per (scenario, iteration) and pooled per (group,
iteration) by an exact selection, per residence when it settled and how far it got, per scenario the stopping rule's
verdict.  Only records are read back.  Drawing stays outside the project."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import BILL_DTYPE, CONV_RES_DTYPE, CONV_RUN_DTYPE, check, ptr
from .bills import check_groups, check_scenarios


@dataclass
class ConvergenceReport:
    """iterations: (S, K) BILL_DTYPE records over the kept residences' diff of scenario s at row k (n_above: the values
    > eps; worst_index: the residence with the largest).  pooled: (G, K), the same over all kept values of a group's
    scenarios.  settle: (S,) BILL_DTYPE records over the kept residences' `settle`.  run: (S,) CONV_RUN_DTYPE --
    converged_at: the first row of `patience` rows whose maximum is within eps (-1: none), last_above, n_unsettled,
    n_never.  residences: (S, n) CONV_RES_DTYPE in the caller's residence order -- max, last, settle (1 + the last row
    above eps; 0: never above; K: not settled within the history), n_above, worst_iteration -- or None (arrays=False).
    groups: (S,) int, -1: in no pool.  keep: (S, n) bool in the caller's order, or None (all)."""
    iterations: np.ndarray
    pooled: np.ndarray
    settle: np.ndarray
    run: np.ndarray
    residences: np.ndarray | None
    eps: float
    patience: int
    groups: np.ndarray
    n_groups: int
    keep: np.ndarray | None = None


def check_conv_args(S, n, K, eps, patience, groups, keep, index=None):
    """The checks of a convergence report, before the device is touched -> (eps float, patience int, group ids int32
    (S,), G, keep uint8 (S, n) or None, index int32 (n,) or None)."""
    check_scenarios("convergence report", S)
    if n < 1 or S * n >= 2 ** 31:
        raise ValueError(f"convergence report: {S} scenarios x {n} residences outside 1..2^31 - 1 columns")
    if K < 1:
        raise ValueError(f"convergence report: the history has {K} rows; it needs at least one")
    eps = float(eps)
    if math.isnan(eps) or eps < 0:
        raise ValueError(f"convergence report: eps = {eps} is negative or a NaN")
    if int(patience) != patience or patience < 1:
        raise ValueError(f"convergence report: patience = {patience!r} must be an integer >= 1")
    patience = min(int(patience), 2 ** 31 - 1)
    gid, G = check_groups(S, groups)
    if G > _lib.STUDY_MAX_S:
        raise ValueError(f"convergence report: group ids up to {G - 1}; a report holds {_lib.STUDY_MAX_S} pools")
    if keep is not None:
        keep = np.asarray(keep)
        if keep.shape != (S, n):
            raise ValueError(f"convergence report: keep must be (scenarios, residences) = {(S, n)}, got {keep.shape}")
        keep = np.ascontiguousarray(keep != 0, np.uint8)
    if index is not None:
        index = np.asarray(index)
        if index.shape != (n,) or not np.issubdtype(index.dtype, np.integer) or index.min() < 0 \
                or index.max() >= 2 ** 31 - 1:
            raise ValueError(f"convergence report: index must be {n} integers in 0..2^31 - 2")
        index = np.ascontiguousarray(index, np.int32)
    return eps, patience, gid, G, keep, index


def convergence_report_device(hist, eps, S=1, keep=None, index=None, groups=None, patience=8, arrays=True, lib=None,
                              stream=None) -> ConvergenceReport:
    """The convergence report of a history that lies on the device: hist a float32 tensor (K, n S) whose last dimension
    is contiguous (a slice of a wider buffer is fine: the row stride is hist.stride(0)); element (k, i S + s) is the diff
    of residence i of scenario s at row k -- the ensemble's sweep layout, with S = 1 an engine's (K, n).  Nothing but the
    side arrays is uploaded; nothing but the records is read back.

    eps       a row of a residence is `above` when !(diff <= eps); a scenario's row is within eps when its largest kept
              diff is.
    keep      None: the records cover every residence.  Else (S, n) booleans, keep[s, i] for ROW i of the history.
    index     None, or n integers: the index worst_index reports for row i (an engine's perm).
    groups    None, or one integer per scenario: the pool it belongs to, 0 .. G-1 with G = max + 1; -1: in none.
    patience  rows within eps in a row that count as converged (AdmmEngine.run's rule).
    arrays    False: the per-residence records are neither computed nor read back (run's two counts are then -1).
    `residences` and `keep` of the result are in the history's row order."""
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.float32 or hist.dim() != 2:
        raise ValueError("convergence report: hist must be a float32 tensor (iterations, residences x scenarios)")
    K, cols = hist.shape
    if K < 1 or cols < 1:
        raise ValueError(f"convergence report: the history is empty, {tuple(hist.shape)}")
    if hist.stride(1) != 1 or (K > 1 and hist.stride(0) < cols):
        raise ValueError("convergence report: the rows of hist must be contiguous and must not overlap")
    if not isinstance(S, (int, np.integer)) or S < 1 or cols % S:
        raise ValueError(f"convergence report: {cols} columns are no multiple of S = {S!r} scenarios")
    S, n = int(S), cols // int(S)
    eps, patience, gid, G, keep, index = check_conv_args(S, n, K, eps, patience, groups, keep, index)
    dev = hist.device
    if dev.type != "cuda":
        raise ValueError(f"convergence report: hist lies on {dev}; the report runs on the GPU")
    ld = hist.stride(0) if K > 1 else cols

    with torch.cuda.device(dev):
        lb = lib or _lib.load()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        d_keep = None if keep is None else torch.from_numpy(keep).to(dev)
        d_index = None if index is None else torch.from_numpy(index).to(dev)
        rec = BILL_DTYPE.itemsize
        u8 = dict(dtype=torch.uint8, device=dev)
        d_iter = torch.empty(S * K * rec, **u8)
        d_pool = torch.empty(G * K * rec, **u8) if G else None
        d_res = torch.empty(S * n * CONV_RES_DTYPE.itemsize, **u8) if arrays else None
        d_run = torch.empty(S * CONV_RUN_DTYPE.itemsize, **u8)
        d_settle = torch.empty(S * rec, **u8)
        nbytes = int(lb.revs_conv_report_scratch(S, n, K, G))
        if nbytes <= 0:
            raise ValueError(f"convergence report: no scratch size for S={S}, {n} residences, {K} rows, {G} groups")
        d_scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        h_group = np.ascontiguousarray(gid, np.int32)
        check(lb.revs_conv_report(S, n, K, ptr(hist), ld, ptr(d_keep), ptr(d_index), h_group.ctypes.data if G else None,
                                  G, eps, patience, ptr(d_iter), ptr(d_pool), ptr(d_res), ptr(d_run), ptr(d_settle),
                                  ptr(d_scratch), st), "revs_conv_report")
        it = d_iter.cpu().numpy().view(BILL_DTYPE).reshape(S, K)
        pool = d_pool.cpu().numpy().view(BILL_DTYPE).reshape(G, K) if G else np.zeros((0, K), BILL_DTYPE)
        res = d_res.cpu().numpy().view(CONV_RES_DTYPE).reshape(S, n) if arrays else None
        run = d_run.cpu().numpy().view(CONV_RUN_DTYPE).reshape(S)
        settle = d_settle.cpu().numpy().view(BILL_DTYPE).reshape(S)
    return ConvergenceReport(it, pool, settle, run, res, eps, patience, gid.astype(np.int64), int(G),
                             None if keep is None else keep != 0)


def convergence_report(diff, eps, keep=None, groups=None, patience=8, arrays=True, device="cuda:0") -> ConvergenceReport:
    """convergence_report_device for a history held on the host: diff (K, n), what solve_ADMM's loop returns, or
    (S, K, n), what AdmmEnsemble.run and solve_ADMM_many's per-solution diff give.  Uploaded once, as float32 in the
    sweep layout (K, n S); keep (S, n) -- or (n,) for one run -- and the records' indices are the caller's."""
    a = np.asarray(diff)
    if a.ndim == 2:
        a = a[None]
        if keep is not None and np.ndim(keep) == 1:
            keep = np.asarray(keep)[None]
    if a.ndim != 3:
        raise ValueError(f"convergence report: diff must be (iterations, residences) or (scenarios, iterations, "
                         f"residences), got {a.shape}")
    S, K, n = a.shape
    check_conv_args(S, n, K, eps, patience, groups, keep)           # (before the device is touched)
    h = np.ascontiguousarray(a.transpose(1, 2, 0), np.float32).reshape(K, n * S)
    from .engine import _dev_check
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        return convergence_report_device(torch.from_numpy(h).to(dev), eps, S, keep, None, groups, patience, arrays)


def report_in_caller_order(rep: ConvergenceReport, inv_perm) -> ConvergenceReport:
    """A report whose rows are an engine's sweep order (index = perm) -> residences and keep in the caller's order."""
    if rep.residences is not None:
        rep.residences = np.ascontiguousarray(rep.residences[:, inv_perm])
    if rep.keep is not None:
        rep.keep = np.ascontiguousarray(rep.keep[:, inv_perm])
    return rep
