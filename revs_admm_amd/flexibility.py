"""The flexibility report: how much of a schedule's charging can still be moved, where and when, without a car leaving
under target -- per EV and slot the largest extra power the battery still takes (up) and the largest cut after which
full-rate charging in the rest of the window still reaches the target (down), per row their sums over the day, the slot
at which the car is ready and the slack it leaves before departure, per slot and per node the reserve of the cars there
-- from the charger power where it lies on the device (revs_flex_report, include/revs_admm_ops.h, DESIGN.md section
3.18): AdmmEngine.S, an ensemble's (n, S, T), the p of a rule schedule.  Only records are read back."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, baselines, row_reports as rr
from ._lib import FLEX_DAY_DTYPE, FLEX_ROW_DTYPE, FLEX_SLOT_DTYPE, check, ptr

WHO = "flexibility report"
QUANTITIES = ("up_energy", "down_energy", "slack", "laxity")
POOLED_SLOT_DTYPE = np.dtype([(k, "<i8") for k in ("n_plugged", "n_up", "n_down")])


@dataclass
class FlexReport:
    """row: (S, n) FLEX_ROW_DTYPE, one record per residence (zeros and ready -1 without an EV), or None (rows=False /
    "device": then row_device is the uint8 tensor of the S n records on the device).  slot: (S, T) FLEX_SLOT_DTYPE; day:
    (S,) FLEX_DAY_DTYPE; hist: (S, 2, T + 1) int32 -- of ready, of slack, over the EV rows that get ready.  node_up /
    node_down: (S, m, T) float64, the reserve of each node's cars per slot -- host arrays (nodes=True), tensors on the
    device (nodes="device") or None.  up_energy / down_energy / slack / laxity: (S,) BILL_DTYPE box-plot records over
    each scenario's EV rows whose power is finite (slack: a car that is never ready counts in n_nan); pooled_*: (G,)
    over all values of a group's scenarios.  pooled_slot (G, T) and pooled_hist (G, 2, T + 1): the members' integer counts
    added up (exact).  groups: (S,) int, -1: in no pool."""
    row: np.ndarray | None
    slot: np.ndarray
    day: np.ndarray
    hist: np.ndarray
    node_up: object | None
    node_down: object | None
    up_energy: np.ndarray
    down_energy: np.ndarray
    slack: np.ndarray
    laxity: np.ndarray
    pooled_up_energy: np.ndarray
    pooled_down_energy: np.ndarray
    pooled_slack: np.ndarray
    pooled_laxity: np.ndarray
    pooled_slot: np.ndarray
    pooled_hist: np.ndarray
    groups: np.ndarray
    n_groups: int
    integral: int
    on_frac: float
    short_tol: float
    row_device: object | None = None

    def up_curve(self):
        """(S, T): the power the scenario's cars could still add in every slot."""
        return self.slot["up"].copy()

    def down_curve(self):
        """(S, T): the power the scenario's cars could still shed in every slot."""
        return self.slot["down"].copy()


def _check_args(S, n, T, groups, on_frac, short_tol, index=None):
    rr.check_sizes(WHO, S, n, T)
    return rr.check_row_args(WHO, S, n, groups, on_frac, short_tol, index)


def flexibility_report_device(p, homes, integral, node_ptr=None, index=None, groups=None, on_frac=0.0, short_tol=1e-6,
                              rows=True, nodes=True, order=None, lib=None, stream=None) -> FlexReport:
    """The report of charger power that lies on the device: p a float32 tensor (n, S, T) or (n, T) whose slots are
    contiguous (the other strides are the tensor's), homes a contiguous uint8 tensor on the same device holding the n S
    revs_home_t records, the record of (i, s) at i S + s -- both as charging_report_device takes them.

    integral  nonzero: on/off chargers (a slot's reserve is the rating or nothing); 0: continuous ones.
    node_ptr  None, or an int64 tensor (m + 1,) on the device: the CSR offsets of the rows sorted by node.  With it and
              nodes=True / "device" the node arrays are reported.
    index, groups, on_frac, short_tol, rows, order: as in charging_report_device."""
    p = rr.check_tensor(WHO, "power", p)
    n, S, T = p.shape
    gid, G, on_frac, short_tol, index = _check_args(S, n, T, groups, on_frac, short_tol, index)
    dev = rr.check_on_device(WHO, p, homes, rows=rows, nodes=nodes)
    m = 0
    if node_ptr is not None and nodes:
        if not isinstance(node_ptr, torch.Tensor) or node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 \
                or node_ptr.numel() < 2 or not node_ptr.is_contiguous() or node_ptr.device != dev:
            raise ValueError(f"flexibility report: node_ptr must be a contiguous int64 tensor (nodes + 1,) on {dev}")
        m = node_ptr.numel() - 1
        if m * S * T >= 2 ** 31:
            raise ValueError(f"flexibility report: {m} nodes x {S} scenarios x {T} slots, 2^31 cells or more")
    with torch.cuda.device(dev):
        lb = lib or _lib.load()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        d_index = None if index is None else torch.from_numpy(index).to(dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        d_row = torch.empty(S * n * FLEX_ROW_DTYPE.itemsize, **u8) if rows else None
        d_slot = torch.empty(S * T * FLEX_SLOT_DTYPE.itemsize, **u8)
        d_day = torch.empty(S * FLEX_DAY_DTYPE.itemsize, **u8)
        d_hist = torch.empty(S, 2, T + 1, dtype=torch.int32, device=dev)
        d_nup = torch.empty(S, m, T, dtype=torch.float64, device=dev) if m else None
        d_ndn = torch.empty(S, m, T, dtype=torch.float64, device=dev) if m else None
        d_val = torch.empty(4, S, n, dtype=torch.float64, device=dev)
        d_keep = torch.empty(S, n, **u8)
        nbytes = int(lb.revs_flex_report_scratch(S, n, T))
        if nbytes <= 0:
            raise ValueError(f"flexibility report: no scratch size for S={S}, {n} residences, T={T}")
        d_scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        check(lb.revs_flex_report(S, n, T, ptr(p), *rr.strides(p), ptr(homes), 1 if integral else 0, on_frac, short_tol,
                                  ptr(node_ptr) if m else None, m, ptr(d_row), ptr(d_slot), ptr(d_day), ptr(d_hist),
                                  ptr(d_nup), ptr(d_ndn), ptr(d_val), ptr(d_keep), ptr(d_scratch), st), "revs_flex_report")
        d_val, d_keep, d_row = rr.reorder(order, d_val, d_keep, d_row)
        box, pool = rr.box_records(lb, st, d_val, d_keep, d_index, gid, G)
        slot = d_slot.cpu().numpy().view(FLEX_SLOT_DTYPE).reshape(S, T)
        day = d_day.cpu().numpy().view(FLEX_DAY_DTYPE).reshape(S)
        hist = d_hist.cpu().numpy()
        row = d_row.cpu().numpy().view(FLEX_ROW_DTYPE).reshape(S, n) if rows is True else None
        if m and nodes is True:
            d_nup, d_ndn = d_nup.cpu().numpy(), d_ndn.cpu().numpy()
    pslot, phist = rr.pooled_counts(slot, hist, gid, G, POOLED_SLOT_DTYPE)
    return FlexReport(row, slot, day, hist, d_nup, d_ndn, *(box[q].copy() for q in range(4)),
                      *(pool[q].copy() for q in range(4)), pslot, phist, gid.astype(np.int64), int(G),
                      1 if integral else 0, on_frac, short_tol, d_row if rows == "device" else None)


def flexibility_report(p, records, integral=0, node_ptr=None, groups=None, on_frac=0.0, short_tol=1e-6, rows=True,
                       nodes=True, device="cuda:0") -> FlexReport:
    """flexibility_report_device for charger power held on the host: p (S, n, T) -- or (n, T) for one schedule -- and
    records HOME_DTYPE (S, n) -- or (n,) -- uploaded once, as float32 in the layout (n, S, T) with the records [n][S];
    node_ptr: None or (m + 1,) integers, the CSR offsets of the rows sorted by node."""
    S, n, T, h, hr = rr.host_rows(WHO, p, records)
    _check_args(S, n, T, groups, on_frac, short_tol)
    if node_ptr is not None:
        node_ptr = np.ascontiguousarray(node_ptr, np.int64)
        if node_ptr.ndim != 1 or len(node_ptr) < 2 or node_ptr[0] != 0 or node_ptr[-1] != n or (np.diff(node_ptr) < 0).any():
            raise ValueError(f"flexibility report: node_ptr must ascend from 0 to {n} residences")
    from .engine import _dev_check
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        d_ptr = None if node_ptr is None else torch.from_numpy(node_ptr).to(dev)
        return flexibility_report_device(torch.from_numpy(h).to(dev), torch.from_numpy(hr).to(dev), integral, d_ptr, None,
                                         groups, on_frac, short_tol, rows, nodes)


class FlexMixin:
    """AdmmEngine.flexibility_report (and, through it, AdmmEnsemble's, on its (n, S, T) view)."""

    def flexibility_report(self, profile=None, groups=None, on_frac=0.0, short_tol=1e-6, rows=True, nodes=True,
                           fill="target", charger=None) -> FlexReport:
        """FlexReport of charger power on the device, for every scenario the engine holds (one; an ensemble: S).

        profile  as in charging_report: None, the charger power S of the last iteration (it raises unless that iteration
                 wrote it); a baselines.POLICIES name, the p of that rule schedule filled to `fill` for `charger`; or a
                 float32 tensor on the device in the engine's residence order, (n, T) -- an ensemble: (n, S, T).
        charger  None: the engine's mode (binary: on/off chargers, else continuous ones); it decides the report's
                 integral flag and the rule schedule's charger.
        nodes    True / "device": node_up and node_down (S, m, T) over the engine's nodes, in the engine's node order (the
                 order of node_sums()), read back or left on the device; False: not computed.
        Row records, indices and the box records are in the caller's residence order; the slot and day sums are sums in
        the ENGINE's order: within the summation bound of those.  Nothing is uploaded, nothing but records is read
        back; the run's state is read, never written."""
        S, n, T = rr.engine_sizes(WHO, self, profile)
        mode = self.mode if charger is None else charger
        integral = baselines.rule_args(profile if isinstance(profile, str) else "uncontrolled", fill, mode)[2]
        _check_args(S, n, T, groups, on_frac, short_tol)                                 # (before any launch)
        p = rr.engine_power(WHO, self, profile, fill, mode)
        inv = torch.from_numpy(np.asarray(self.inv_perm, np.int64)).to(self.S.device)
        return flexibility_report_device(p, self.homes.view(-1), integral, self.node_ptr if nodes else None, None, groups,
                                         on_frac, short_tol, rows, nodes, order=inv, lib=self.lib, stream=self.stream)
