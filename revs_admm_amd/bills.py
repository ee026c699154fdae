"""The bill report: what schedules cost each residence under the tariff, and their deviation from a baseline schedule
-- the reference's last result figure (test-centralopt.py:112-116: per EV residence C = sum_t P_res[t] COST[t] for two
schedules, dev = 100 (C2 - C1) / C1), for the S scenarios of a study at once on the GPU (revs_bill_rows /
revs_bill_study, include/revs_admm_ops.h): bills and deviations per (scenario, residence),
box-plot records per scenario and pooled over groups by an exact selection, and per residence the statistics of the
deviation ACROSS a group's scenarios (BillReport.across, through revs_net_across).  Drawing stays outside the project."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import BILL_DTYPE, check, ptr


@dataclass
class BillReport:
    """bill, dev: (S, n) float64 -- bill[s, i] = sum_t tariff[t] g[s, i, t] in slot order, one accumulator;
    dev[s, i] = 100 (bill[s, i] - bill[base[s], i]) / bill[base[s], i], NaN where base[s] == -1 -- or None
    (arrays=False).  summary_bill / summary_dev: (S,) BILL_DTYPE records over scenario s's kept residences;
    pooled_bill / pooled_dev: (G,) over all kept values of a group's scenarios.  base, groups: (S,) int, -1: no
    baseline / in no pool.  keep: (S, n) bool, the residences the records cover, or None (all)."""
    bill: np.ndarray | None
    dev: np.ndarray | None
    summary_bill: np.ndarray
    summary_dev: np.ndarray
    pooled_bill: np.ndarray
    pooled_dev: np.ndarray
    base: np.ndarray
    groups: np.ndarray
    n_groups: int
    keep: np.ndarray | None = None
    device: str = "cuda:0"

    def across(self, groups=None):
        """(G, n) ACROSS_DTYPE records: per residence the statistics of dev ACROSS the scenarios of each group
        (default: the report's groups) -- count scenarios with a deviation, n_violations of them above 0 (the residence
        pays more than under the baseline), min .. max, mean, the worst scenario.  Residences a scenario does not keep
        count as NaN there.  revs_net_across with T = 1, sense +1, lo = -inf, hi = 0: at most 65535 residences."""
        from .study import native_across
        if self.dev is None:
            raise ValueError("bill report: across() needs the deviations (arrays=True)")
        S, n = self.dev.shape
        gid, G = check_groups(S, self.groups if groups is None else groups)
        if G < 1:
            raise ValueError("bill report: across() needs groups with at least one scenario in one")
        if n > 0xFFFF:
            raise ValueError(f"bill report: across() holds 65535 residences, got {n}")
        v = self.dev if self.keep is None else np.where(self.keep, self.dev, np.nan)
        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            d_v = torch.from_numpy(np.ascontiguousarray(v, np.float64).reshape(S, n, 1)).to(dev)
            slot, _, _ = native_across(_lib.load(), torch.cuda.current_stream(dev).cuda_stream, d_v, None, gid, G,
                                       -np.inf, 0.0, 1, (), True)
        return slot[:, :, 0].copy()


def check_scenarios(who, S):
    """The bound on the scenarios of one call that every report shares; `who`: the report's name in front of the message."""
    if not 1 <= S <= _lib.STUDY_MAX_S:
        raise ValueError(f"{who}: {S} scenarios outside 1..{_lib.STUDY_MAX_S}")


def check_groups(S, groups):
    """-> (group ids int32 (S,), G)."""
    if groups is None:
        return np.full(S, -1, np.int32), 0
    gid = np.asarray(groups)
    if gid.shape != (S,) or not np.issubdtype(gid.dtype, np.integer) or gid.min() < -1:
        raise ValueError(f"bill report: groups must be {S} integers >= -1")
    return gid.astype(np.int32), int(gid.max()) + 1


def check_bill_args(S, n, T, tariff, base, groups, keep):
    """The checks of a bill report, before the device is touched -> (tariff float64 (T,), base int32 (S,), group ids
    int32 (S,), G, keep uint8 (S, n) or None)."""
    check_scenarios("bill report", S)
    if not 1 <= T <= _lib.MAX_T:
        raise ValueError(f"bill report: {T} slots outside 1..{_lib.MAX_T}")
    if n < 1 or S * n >= 2 ** 31:
        raise ValueError(f"bill report: {S} scenarios x {n} residences outside 1..2^31 - 1 rows")
    tariff = np.ascontiguousarray(tariff, np.float64)
    if tariff.shape != (T,):
        raise ValueError(f"bill report: the tariff must have one price per slot ({T}), got {tariff.shape}")
    if base is None:
        base = np.full(S, -1, np.int32)
    else:
        base = np.asarray(base)
        if base.shape != (S,) or not np.issubdtype(base.dtype, np.integer) or base.min() < -1 or base.max() >= S:
            raise ValueError(f"bill report: base must be {S} integers in -1..{S - 1}")
        base = base.astype(np.int32)
    gid, G = check_groups(S, groups)
    if keep is not None:
        keep = np.asarray(keep)
        if keep.shape != (S, n):
            raise ValueError(f"bill report: keep must be (scenarios, residences) = {(S, n)}, got {keep.shape}")
        keep = np.ascontiguousarray(keep != 0, np.uint8)
    return tariff, base, gid, G, keep


def native_bill_study(lib, stream, d_bill, base, d_keep, d_index, gid, G, arrays) -> BillReport:
    """revs_bill_study on bills that lie on the device: d_bill (S, n) float64 device tensor, base / gid (S,) int32 on
    the host, d_keep (S, n) uint8 device tensor or None, d_index (n,) int32 device tensor or None (the index worst_index
    reports for every row).  The records -- and with arrays=True the bills and deviations -- are read back."""
    S, n = d_bill.shape
    dev = d_bill.device
    rec = BILL_DTYPE.itemsize
    d_sum = torch.empty(S * 2 * rec, dtype=torch.uint8, device=dev)
    d_pool = torch.empty(G * 2 * rec, dtype=torch.uint8, device=dev) if G else None
    d_dev = torch.empty(S, n, dtype=torch.float64, device=dev) if arrays else None
    nbytes = int(lib.revs_bill_study_scratch(S, n))
    if nbytes <= 0:
        raise ValueError(f"bill report: no scratch size for S={S}, {n} residences")
    d_scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    h_base, h_group = np.ascontiguousarray(base, np.int32), np.ascontiguousarray(gid, np.int32)
    check(lib.revs_bill_study(S, n, ptr(d_bill), h_base.ctypes.data, ptr(d_keep), ptr(d_index),
                              h_group.ctypes.data if G else None, G, ptr(d_dev), ptr(d_sum), ptr(d_pool),
                              ptr(d_scratch), stream), "revs_bill_study")
    s = d_sum.cpu().numpy().view(BILL_DTYPE).reshape(S, 2)
    p = d_pool.cpu().numpy().view(BILL_DTYPE).reshape(G, 2) if G else np.zeros((0, 2), BILL_DTYPE)
    bill = dev_ = keep = None
    if arrays:
        bill, dev_ = d_bill.cpu().numpy(), d_dev.cpu().numpy()
    if d_keep is not None:
        keep = d_keep.cpu().numpy() != 0
    return BillReport(bill, dev_, s[:, 0].copy(), s[:, 1].copy(), p[:, 0].copy(), p[:, 1].copy(),
                      h_base.astype(np.int64), h_group.astype(np.int64), int(G), keep, str(dev))


def bill_report_device(g, tariff, base=None, groups=None, keep=None, arrays=True, lib=None, stream=None) -> BillReport:
    """The bill report of S schedules that lie on the device: g a contiguous (S, n, T) float32 or float64 tensor, the
    net load of residence i of scenario s; tariff (T,) prices.  Nothing but the side arrays is uploaded.

    base      None: bills only (every deviation a NaN).  Else one integer per scenario: the scenario whose bills are its
              baseline, -1: none.
    groups    None, or one integer per scenario: the pool it belongs to, 0 .. G-1 with G = max + 1; -1: in none.
    keep      None: the records cover every residence.  Else (S, n) booleans: those of scenario s with keep[s, i].
    arrays    False: the records alone are read back."""
    if not isinstance(g, torch.Tensor) or g.dtype not in (torch.float32, torch.float64) or g.dim() != 3 \
            or not g.is_contiguous():
        raise ValueError("bill report: g must be a contiguous (scenarios, residences, slots) float32 or float64 tensor")
    S, n, T = g.shape
    tariff, base, gid, G, keep = check_bill_args(S, n, T, tariff, base, groups, keep)
    dev = g.device

    def run():
        lb = lib or _lib.load()
        st = stream
        if st is None and dev.type == "cuda":
            st = torch.cuda.current_stream(dev).cuda_stream
        d_tariff = torch.from_numpy(tariff).to(dev)
        d_keep = None if keep is None else torch.from_numpy(keep).to(dev)
        d_bill = torch.empty(S, n, dtype=torch.float64, device=dev)
        check(lb.revs_bill_rows(S, n, T, ptr(g), int(g.dtype == torch.float64), n * T, T, ptr(d_tariff), ptr(d_bill), st),
              "revs_bill_rows")
        return native_bill_study(lb, st, d_bill, base, d_keep, None, gid, G, arrays)

    if dev.type != "cuda":
        raise ValueError(f"bill report: g lies on {dev}; the report runs on the GPU")
    with torch.cuda.device(dev):
        return run()


def bill_report(profiles, tariff, base=None, groups=None, keep=None, arrays=True, device="cuda:0") -> BillReport:
    """bill_report_device for schedules held on the host: profiles (S, n, T), uploaded as float64 (float32 arrays as
    float32: the bills widen every value first, so the bits are the same)."""
    a = np.asarray(profiles)
    if a.ndim != 3:
        raise ValueError(f"bill report: profiles must be (scenarios, residences, slots), got {a.shape}")
    a = np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64)
    check_bill_args(*a.shape, tariff, base, groups, keep)           # (before the device is touched)
    from .engine import _dev_check
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        return bill_report_device(torch.from_numpy(a).to(dev), tariff, base, groups, keep, arrays)
