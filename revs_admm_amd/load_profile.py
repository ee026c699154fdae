"""The load-profile report: the demand curve of a schedule -- the residences' load per slot as a box-plot record, the
feeder's peak and its slot, how flat the day is, how the residences' own peaks add up against it, each for the
residences with and without an EV (or any other classes) and for all of them -- what the reference draws in
test-altered-profile.py:25-57, on the GPU from the schedule where it lies (revs_load_profile, include/revs_admm_ops.h,
DESIGN.md section 3.13).  Only records are read back.  Drawing stays outside the project."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, baselines, row_reports as rr
from ._lib import BILL_DTYPE, PROFILE_DAY_DTYPE, check, ptr

WHO = "load profile"


@dataclass
class LoadProfileReport:
    """slot: (S, Q, T) BILL_DTYPE records over the set's loads at slot t (total: the aggregate; n_above: the values >
    `above`; worst_index: the residence with the largest).  peak: (S, Q), the same over every residence's own daily peak.
    day: (S, Q) PROFILE_DAY_DTYPE -- peak / valley of the aggregate and their slots, energy, load_factor, sum_peaks,
    diversity.  pooled_slot (G, Q, T) / pooled_peak (G, Q): the records over all values of a group's scenarios.
    classes: the Q set names, the last one "all".  groups: (S,) int, -1: in no pool."""
    slot: np.ndarray
    peak: np.ndarray
    day: np.ndarray
    pooled_slot: np.ndarray
    pooled_peak: np.ndarray
    classes: tuple
    groups: np.ndarray
    n_groups: int
    above: float

    def aggregate(self):
        """(S, Q, T): the set's total load per slot (NaN where the set holds no value)."""
        return self.slot["total"].copy()

    def mean(self):
        """(S, Q, T): total / count, the line the reference draws."""
        with np.errstate(all="ignore"):
            return self.slot["total"] / self.slot["count"]

    def peak_change(self, other: "LoadProfileReport"):
        """(S, Q): 100 (peak - other's peak) / other's peak of the aggregate, per scenario and set."""
        with np.errstate(all="ignore"):
            return 100 * (self.day["peak"] - other.day["peak"]) / other.day["peak"]

    def group_day_mean(self):
        """dict of (G, Q) arrays: the mean over a group's scenarios of every double of `day` (NaN: no member has one)."""
        out = {}
        for k in ("peak", "valley", "energy", "load_factor", "sum_peaks", "diversity"):
            a = np.full((self.n_groups,) + self.day.shape[1:], np.nan)
            for g in range(self.n_groups):
                m = self.day[k][self.groups == g]
                ok = ~np.isnan(m)
                with np.errstate(all="ignore"):
                    a[g] = np.where(ok.any(0), np.where(ok, m, 0.0).sum(0) / ok.sum(0), np.nan)
            out[k] = a
        return out


def check_profile_args(S, n, T, classes, n_classes, groups, above, index=None, names=None):
    """The checks of a load-profile report, before the library is loaded -> (class bytes uint8 (S, n) or None, C, set
    names, group ids int32 (S,), G, above float, index int32 (n,) or None).  classes: None (one set: everybody), or
    integers (S, n) -- (n,) with S == 1 -- where 0 .. C-1 is a class and anything else (negative, >= C) leaves the
    residence out; n_classes: C, default 1 + the largest entry in 0 .. PROFILE_MAX_CLASSES - 1."""
    rr.check_sizes(WHO, S, n, T)
    above = float(above)
    if math.isnan(above):
        raise ValueError("load profile: above is a NaN")
    gid, G = rr.check_pools(WHO, S, groups)
    cls, C = None, 0
    if classes is not None:
        a = np.asarray(classes)
        if a.ndim == 1 and S == 1:
            a = a[None]
        if a.shape != (S, n) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == bool):
            raise ValueError(f"load profile: classes must be integers (scenarios, residences) = {(S, n)}, got "
                             f"{a.dtype} {a.shape}")
        a = a.astype(np.int64)
        inside = a[(a >= 0) & (a < _lib.PROFILE_MAX_CLASSES)]
        C = int(n_classes) if n_classes is not None else int(inside.max()) + 1 if inside.size else 1
        if not 1 <= C <= _lib.PROFILE_MAX_CLASSES:
            raise ValueError(f"load profile: {C} classes outside 1..{_lib.PROFILE_MAX_CLASSES}")
        cls = np.ascontiguousarray(np.where((a >= 0) & (a < C), a, 255), np.uint8)
    elif n_classes not in (None, 0):
        raise ValueError(f"load profile: {n_classes} classes without a class per residence")
    if names is None:
        names = tuple(f"class {c}" for c in range(C))
    names = tuple(names)
    if len(names) != C:
        raise ValueError(f"load profile: {len(names)} names for {C} classes")
    return cls, C, names + ("all",), gid, G, above, rr.check_index(WHO, n, index)


def load_profile_report_device(g, classes=None, n_classes=None, names=None, index=None, groups=None, above=0.0, lib=None,
                               stream=None) -> LoadProfileReport:
    """The report of a profile that lies on the device: g a float32 tensor (n, S, T) or (n, T) whose slots are contiguous
    (the other strides are the tensor's: a view of a wider buffer is fine) -- an ensemble's layout, what rule_schedule()
    returns.  classes: None, integers (S, n) on the host, or a uint8 tensor (S, n) on the device (then n_classes is
    needed; a byte >= n_classes leaves the residence out).  index: the index worst_index reports for row i.  Nothing but
    the class bytes and the index is uploaded; nothing but the records is read back."""
    g = rr.check_tensor(WHO, "profile", g)
    n, S, T = g.shape
    on_dev = isinstance(classes, torch.Tensor)
    if on_dev:
        if classes.dtype != torch.uint8 or tuple(classes.shape) != (S, n) or not classes.is_contiguous() or not n_classes:
            raise ValueError(f"load profile: classes on the device must be a contiguous uint8 tensor {(S, n)}, with n_classes")
    cls, C, sets, gid, G, above, index = check_profile_args(S, n, T, None if on_dev else classes,
                                                            None if on_dev else n_classes, groups, above, index,
                                                            None if on_dev else names)
    if on_dev:
        C = int(n_classes)
        if not 1 <= C <= _lib.PROFILE_MAX_CLASSES:
            raise ValueError(f"load profile: {C} classes outside 1..{_lib.PROFILE_MAX_CLASSES}")
        sets = (tuple(names) if names is not None else tuple(f"class {c}" for c in range(C))) + ("all",)
        if len(sets) != C + 1:
            raise ValueError(f"load profile: {len(sets) - 1} names for {C} classes")
    dev = g.device
    if dev.type != "cuda":
        raise ValueError(f"load profile: the profile lies on {dev}; the report runs on the GPU")
    Q = C + 1
    with torch.cuda.device(dev):
        lb = lib or _lib.load()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        d_cls = classes if on_dev else None if cls is None else torch.from_numpy(cls).to(dev)
        d_index = None if index is None else torch.from_numpy(index).to(dev)
        rec = BILL_DTYPE.itemsize
        u8 = dict(dtype=torch.uint8, device=dev)
        d_slot, d_peak = torch.empty(S * Q * T * rec, **u8), torch.empty(S * Q * rec, **u8)
        d_day = torch.empty(S * Q * PROFILE_DAY_DTYPE.itemsize, **u8)
        d_pslot = torch.empty(G * Q * T * rec, **u8) if G else None
        d_ppeak = torch.empty(G * Q * rec, **u8) if G else None
        nbytes = int(lb.revs_load_profile_scratch(S, n, T, C, G))
        if nbytes <= 0:
            raise ValueError(f"load profile: no scratch size for S={S}, {n} residences, T={T}, {C} classes, {G} groups")
        d_scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        h_group = np.ascontiguousarray(gid, np.int32)
        check(lb.revs_load_profile(S, n, T, ptr(g), *rr.strides(g), ptr(d_cls), C, ptr(d_index),
                                   h_group.ctypes.data if G else None, G, above, ptr(d_slot), ptr(d_peak), ptr(d_day),
                                   ptr(d_pslot), ptr(d_ppeak), ptr(d_scratch), st), "revs_load_profile")
        slot = d_slot.cpu().numpy().view(BILL_DTYPE).reshape(S, Q, T)
        peak = d_peak.cpu().numpy().view(BILL_DTYPE).reshape(S, Q)
        day = d_day.cpu().numpy().view(PROFILE_DAY_DTYPE).reshape(S, Q)
        pslot = d_pslot.cpu().numpy().view(BILL_DTYPE).reshape(G, Q, T) if G else np.zeros((0, Q, T), BILL_DTYPE)
        ppeak = d_ppeak.cpu().numpy().view(BILL_DTYPE).reshape(G, Q) if G else np.zeros((0, Q), BILL_DTYPE)
    return LoadProfileReport(slot, peak, day, pslot, ppeak, sets, gid.astype(np.int64), int(G), above)


def load_profile_report(g, classes=None, n_classes=None, names=None, groups=None, above=0.0,
                        device="cuda:0") -> LoadProfileReport:
    """load_profile_report_device for profiles held on the host: g (S, n, T) -- or (n, T) for one schedule -- uploaded
    once, as float32 in the layout (n, S, T).  classes (S, n) or (n,); the records' indices are the caller's."""
    a = np.asarray(g)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.size == 0:
        raise ValueError(f"load profile: g must be (residences, slots) or (scenarios, residences, slots), got {a.shape}")
    S, n, T = a.shape
    if classes is not None and np.ndim(classes) == 1 and S > 1:
        classes = np.broadcast_to(np.asarray(classes)[None], (S, n))
    check_profile_args(S, n, T, classes, n_classes, groups, above, None, names)       # (before the device is touched)
    h = np.ascontiguousarray(a.transpose(1, 0, 2), np.float32)
    from .engine import _dev_check
    dev = _dev_check(device)
    with torch.cuda.device(dev):
        return load_profile_report_device(torch.from_numpy(h).to(dev), classes, n_classes, names, None, groups, above)


class LoadProfileMixin:
    """AdmmEngine.load_profile_report (and, through it, AdmmEnsemble's, on its (n, S, T) view)."""

    def load_profile_report(self, profile=None, classes="ev", groups=None, above=None) -> LoadProfileReport:
        """LoadProfileReport of a profile on the device, for every scenario the engine holds (one; an ensemble: S).

        profile  None: the schedules P_sch.  "load": the base load the sweep holds.  A baselines.POLICIES name
                 ("uncontrolled", "last_minute", "trickle"): self.rule_schedule(name).  A float32 tensor on the device in
                 the form rule_schedule() returns -- (n, T), an ensemble's (n, S, T), the engine's residence order.
        classes  "ev": class 0 "without EV", class 1 "with EV", from the `ev` word of the records on the device.  None:
                 one set.  Or integers in the caller's residence order, (n,) -- an ensemble: (S, n) -- 0 .. C-1.
        groups   None, or one integer per scenario: the pool it belongs to; -1: in none.
        above    n_above counts the loads > above (default 0.0: the residences that draw power).
        worst_index is in the caller's residence order (index_of_row is the engine's perm).  Nothing is read back but
        records, nothing is reordered, nothing is uploaded beyond the class bytes and the index; the run's state is read,
        never written.  `total` is summed in the ENGINE's residence order: it agrees with load_profile_report() on
        result()'s schedules within the summation bound (count 2^-53 sum|x|), while every selected field -- counts,
        extremes, quartiles, whiskers, fliers, the worst entry -- agrees bit for bit.  A sharded engine (group=) reports
        its own rank's residences only."""
        shape = self._rule_shape()
        n, T = shape[0], shape[-1]
        S = shape[1] if len(shape) == 3 else 1
        if isinstance(profile, str) and profile != "load" and profile not in baselines.POLICIES:
            raise ValueError(f'load profile: profile must be None, "load", one of {sorted(baselines.POLICIES)} or a tensor '
                             f'on the device, got {profile!r}')
        if isinstance(classes, str) and classes != "ev":
            raise ValueError(f'load profile: classes must be "ev", None or integers per residence, got {classes!r}')
        above = 0.0 if above is None else above
        ev = isinstance(classes, str)
        host_cls = None if ev or classes is None else np.asarray(classes)
        if host_cls is not None:
            if host_cls.ndim == 1 and S > 1:
                host_cls = np.broadcast_to(host_cls[None], (S, n))
            if host_cls.shape not in ((n,), (S, n)):
                raise ValueError(f"load profile: classes must be one integer per residence, {(S, n)}, got {host_cls.shape}")
            host_cls = host_cls.reshape(S, n)[:, self.perm]
        check_profile_args(S, n, T, host_cls, None, groups, above, np.asarray(self.perm))   # (before any launch)
        if profile is None:
            g = self.P_sch.view(shape)
        elif isinstance(profile, str):
            g = self.load.view(shape) if profile == "load" else self.rule_schedule(profile)
        else:
            g = profile
            if not isinstance(g, torch.Tensor) or tuple(g.shape) != tuple(shape) or g.device != self.P_sch.device:
                raise ValueError(f"load profile: a profile tensor must be {tuple(shape)} on {self.P_sch.device}, the form "
                                 f"rule_schedule() returns")
        names = None
        d_cls, C = host_cls, None
        if ev:                                     # (ev: the first int32 of a 32-byte record; records are [n][S])
            d_cls = (self.homes.view(torch.int32).view(n * S, -1)[:, 0].view(n, S).t() != 0).to(torch.uint8).contiguous()
            C, names = 2, ("without EV", "with EV")
        return load_profile_report_device(g, d_cls, C, names, np.asarray(self.perm), groups, above, lib=self.lib,
                                          stream=self.stream)
