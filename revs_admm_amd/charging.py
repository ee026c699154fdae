"""The charging report: what the chargers do, per EV and per slot -- when the cars start charging and how long they wait
after arrival, how many chargers run at the same moment, how often a session is interrupted, whether each car leaves at
its target state of charge and what the charging cost it -- from the charger power where it lies on the device
(revs_charge_report, include/revs_admm_ops.h): the reference's ev_schedule, AdmmEngine.S, an
ensemble's (n, S, T), the p of a rule schedule.  Only records are read back.  Drawing stays outside the project."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, baselines, row_reports as rr
from ._lib import CHARGE_DAY_DTYPE, CHARGE_ROW_DTYPE, CHARGE_SLOT_DTYPE, check, ptr

WHO = "charging report"
QUANTITIES = ("energy", "cost", "soc_end", "wait")
POOLED_SLOT_DTYPE = np.dtype([(k, "<i8") for k in ("n_ev", "n_plugged", "n_on", "n_full", "n_starts")])


@dataclass
class ChargingReport:
    """row: (S, n) CHARGE_ROW_DTYPE, one record per residence (zeros without an EV), or None (rows=False / "device": then
    row_device is the uint8 tensor of the S n records on the device).  slot: (S, T) CHARGE_SLOT_DTYPE; day: (S,)
    CHARGE_DAY_DTYPE; hist: (S, 3, T + 1) int32 -- of n_on, of wait, of sessions, over the EV rows.  energy / cost /
    soc_end / wait: (S,) BILL_DTYPE box-plot records over each scenario's EV rows whose power is finite (wait: a charger
    that is never on counts in n_nan); pooled_*: (G,) over all values of a group's scenarios.  pooled_slot (G, T) and
    pooled_hist (G, 3, T + 1): the members' integer counts added up (exact).  groups: (S,) int, -1: in no pool."""
    row: np.ndarray | None
    slot: np.ndarray
    day: np.ndarray
    hist: np.ndarray
    energy: np.ndarray
    cost: np.ndarray
    soc_end: np.ndarray
    wait: np.ndarray
    pooled_energy: np.ndarray
    pooled_cost: np.ndarray
    pooled_soc_end: np.ndarray
    pooled_wait: np.ndarray
    pooled_slot: np.ndarray
    pooled_hist: np.ndarray
    groups: np.ndarray
    n_groups: int
    on_frac: float
    short_tol: float
    row_device: object | None = None

    def on_curve(self):
        """(S, T): the chargers that are on in every slot."""
        return self.slot["n_on"].copy()

    def coincidence(self):
        """(S, T): the share of the scenario's chargers that are on in every slot (NaN without an EV)."""
        with np.errstate(all="ignore"):
            return self.slot["n_on"] / np.where(self.slot["n_ev"] > 0, self.slot["n_ev"], np.nan)

    def compare(self, other: "ChargingReport"):
        """dict of (S,) arrays, this report against `other` (the before of a study): the change of peak_on, of peak_power,
        of the mean wait (wait's total / count) and of the cost per scenario."""
        with np.errstate(all="ignore"):
            mean = lambda r: r.wait["total"] / r.wait["count"]
            return dict(peak_on=self.day["peak_on"].astype(np.int64) - other.day["peak_on"],
                        peak_power=self.day["peak_power"] - other.day["peak_power"],
                        wait=mean(self) - mean(other), cost=self.day["cost"] - other.day["cost"])


def check_charge_args(S, n, T, tariff, groups, on_frac, short_tol, index=None):
    """The checks of a charging report, before the library is loaded -> (tariff float64 (T,) or None, group ids int32
    (S,), G, on_frac, short_tol, index int32 (n,) or None).  A tariff that is a tensor on the device passes as it is."""
    rr.check_sizes(WHO, S, n, T)
    if isinstance(tariff, torch.Tensor):
        if tariff.dtype != torch.float64 or tuple(tariff.shape) != (T,) or not tariff.is_contiguous():
            raise ValueError(f"charging report: a tariff on the device must be a contiguous float64 tensor ({T},)")
    elif tariff is not None:
        tariff = np.ascontiguousarray(tariff, np.float64)
        if tariff.shape != (T,):
            raise ValueError(f"charging report: the tariff must have one price per slot ({T}), got {tariff.shape}")
    return (tariff,) + rr.check_row_args(WHO, S, n, groups, on_frac, short_tol, index)


def charging_report_device(p, homes, tariff=None, index=None, groups=None, on_frac=0.0, short_tol=1e-6, rows=True,
                           order=None, lib=None, stream=None) -> ChargingReport:
    """The report of charger power that lies on the device: p a float32 tensor (n, S, T) or (n, T) whose slots are
    contiguous (the other strides are the tensor's: a view of a wider buffer is fine) -- an ensemble's layout, the p of
    rule_schedule_device.  homes: a contiguous uint8 tensor on the same device holding the n S revs_home_t records
    (HOME_DTYPE bytes), the record of (i, s) at i S + s.  tariff: (T,) prices on the host, a float64 tensor on the device,
    or None: every cost is then a NaN.

    index     the index worst_index reports for row i (default i).
    groups    None, or one integer per scenario: the pool it belongs to, 0 .. G-1; -1: in none.
    on_frac   a slot is on when p > on_frac * rating.
    short_tol a car leaves under target when max(0.9, initial) - soc_end > short_tol.
    rows      True: the S n row records are read back.  "device": they stay on the device (row_device).  False: they are
              not written at all.
    order     None, or an int64 tensor on the device: the rows are reported in the order i -> order[i] (row records,
              and the box records' totals: those are sums in the order of the rows)."""
    p = rr.check_tensor(WHO, "power", p)
    n, S, T = p.shape
    tariff, gid, G, on_frac, short_tol, index = check_charge_args(S, n, T, tariff, groups, on_frac, short_tol, index)
    dev = rr.check_on_device(WHO, p, homes, rows=rows)
    with torch.cuda.device(dev):
        lb = lib or _lib.load()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        d_tariff = tariff if tariff is None or isinstance(tariff, torch.Tensor) else torch.from_numpy(tariff).to(dev)
        d_index = None if index is None else torch.from_numpy(index).to(dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        d_row = torch.empty(S * n * CHARGE_ROW_DTYPE.itemsize, **u8) if rows else None
        d_slot = torch.empty(S * T * CHARGE_SLOT_DTYPE.itemsize, **u8)
        d_day = torch.empty(S * CHARGE_DAY_DTYPE.itemsize, **u8)
        d_hist = torch.empty(S, 3, T + 1, dtype=torch.int32, device=dev)
        d_val = torch.empty(4, S, n, dtype=torch.float64, device=dev)
        d_keep = torch.empty(S, n, **u8)
        nbytes = int(lb.revs_charge_report_scratch(S, n, T))
        if nbytes <= 0:
            raise ValueError(f"charging report: no scratch size for S={S}, {n} residences, T={T}")
        d_scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        check(lb.revs_charge_report(S, n, T, ptr(p), *rr.strides(p), ptr(homes), ptr(d_tariff), on_frac, short_tol,
                                    ptr(d_row), ptr(d_slot), ptr(d_day), ptr(d_hist), ptr(d_val), ptr(d_keep),
                                    ptr(d_scratch), st), "revs_charge_report")
        d_val, d_keep, d_row = rr.reorder(order, d_val, d_keep, d_row)
        box, pool = rr.box_records(lb, st, d_val, d_keep, d_index, gid, G)
        slot = d_slot.cpu().numpy().view(CHARGE_SLOT_DTYPE).reshape(S, T)
        day = d_day.cpu().numpy().view(CHARGE_DAY_DTYPE).reshape(S)
        hist = d_hist.cpu().numpy()
        row = d_row.cpu().numpy().view(CHARGE_ROW_DTYPE).reshape(S, n) if rows is True else None
    pslot, phist = rr.pooled_counts(slot, hist, gid, G, POOLED_SLOT_DTYPE)
    return ChargingReport(row, slot, day, hist, *(box[q].copy() for q in range(4)), *(pool[q].copy() for q in range(4)),
                          pslot, phist, gid.astype(np.int64), int(G), on_frac, short_tol,
                          d_row if rows == "device" else None)


def charging_report(p, records, tariff=None, groups=None, on_frac=0.0, short_tol=1e-6, rows=True,
                    device="cuda:0") -> ChargingReport:
    """charging_report_device for charger power held on the host: p (S, n, T) -- or (n, T) for one schedule -- and
    records HOME_DTYPE (S, n) -- or (n,) -- uploaded once, as float32 in the layout (n, S, T) with the records [n][S]."""
    S, n, T, h, hr = rr.host_rows(WHO, p, records)
    check_charge_args(S, n, T, None if isinstance(tariff, torch.Tensor) else tariff, groups, on_frac, short_tol)
    from .engine import _dev_check
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        return charging_report_device(torch.from_numpy(h).to(dev), torch.from_numpy(hr).to(dev), tariff, None, groups,
                                      on_frac, short_tol, rows)


class ChargingMixin:
    """AdmmEngine.charging_report (and, through it, AdmmEnsemble's, on its (n, S, T) view)."""

    _sc_iteration = -1                             # the iteration whose sweep wrote S and Csoc (step(write_sc=True))

    def charging_report(self, profile=None, tariff="engine", groups=None, on_frac=0.0, short_tol=1e-6, rows=True,
                        fill="target", charger=None) -> ChargingReport:
        """ChargingReport of charger power on the device, for every scenario the engine holds (one; an ensemble: S).

        profile  None: the charger power S of the last iteration; it raises unless that iteration wrote it (step() does,
                 run() in its last iteration, run_steps() does not).  A baselines.POLICIES name ("uncontrolled",
                 "last_minute", "trickle"): the p of that rule schedule on the records the sweep holds, filled to `fill`
                 for `charger` (default: the engine's mode).  A float32 tensor on the device in the engine's residence
                 order, (n, T) -- an ensemble: (n, S, T).
        tariff   "engine": the prices the sweep runs on, widened.  None: no costs.  Or (T,) prices.
        Row records, indices and the box records are in the caller's residence order (the values are put into it on the
        device before they are summarised, so they are bit for bit what charging_report() gives on result()'s S); the
        slots' power and the day's energy and cost are sums in the ENGINE's order: within the summation bound of those.
        Nothing is uploaded, nothing but records is read back; the run's state is read, never written."""
        S, n, T = rr.engine_sizes(WHO, self, profile)
        charger = self.mode if charger is None else charger
        if isinstance(profile, str):
            baselines.rule_args(profile, fill, charger)
        host_tariff = None if isinstance(tariff, str) or isinstance(tariff, torch.Tensor) else tariff
        if isinstance(tariff, str) and tariff != "engine":
            raise ValueError(f'charging report: tariff must be "engine", None or one price per slot, got {tariff!r}')
        check_charge_args(S, n, T, host_tariff, groups, on_frac, short_tol)              # (before any launch)
        p = rr.engine_power(WHO, self, profile, fill, charger)
        if isinstance(tariff, str):
            assert self.cost.numel() == T
            tariff = self.cost.double()
        inv = torch.from_numpy(np.asarray(self.inv_perm, np.int64)).to(self.S.device)
        return charging_report_device(p, self.homes.view(-1), tariff, None, groups, on_frac, short_tol, rows, order=inv,
                                      lib=self.lib, stream=self.stream)
