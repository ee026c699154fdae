"""What the reports over the residences' rows stage alike before and after their one call into the library (charging.py,
flexibility.py; load_profile.py uses the checks and the strides): the argument checks, the two strides, the reordering
into the caller's residence order, the box records, the pooled counts, a host caller's upload and an engine's choice of
profile.  Plain functions; `who` is the report's name in front of every message ("charging report")."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, baselines
from ._lib import BILL_DTYPE, HOME_DTYPE, check, ptr
from .bills import check_groups, check_scenarios


def check_sizes(who, S, n, T):
    check_scenarios(who, S)
    if not 1 <= T <= _lib.MAX_T:
        raise ValueError(f"{who}: {T} slots outside 1..{_lib.MAX_T}")
    if n < 1 or S * n >= 2 ** 31:
        raise ValueError(f"{who}: {S} scenarios x {n} residences outside 1..2^31 - 1 rows")


def check_pools(who, S, groups):
    """-> (group ids int32 (S,), G)."""
    gid, G = check_groups(S, groups)
    if G > S:
        raise ValueError(f"{who}: group ids up to {G - 1} for {S} scenarios")
    return gid, G


def check_index(who, n, index):
    """-> index as contiguous int32 (n,), or None."""
    if index is None:
        return None
    index = np.asarray(index)
    if index.shape != (n,) or not np.issubdtype(index.dtype, np.integer) or index.min() < 0 or index.max() >= 2 ** 31 - 1:
        raise ValueError(f"{who}: index must be {n} integers in 0..2^31 - 2")
    return np.ascontiguousarray(index, np.int32)


def check_row_args(who, S, n, groups, on_frac, short_tol, index=None):
    """The checks of a report over EV rows behind check_sizes, before the library is loaded -> (group ids int32 (S,), G,
    on_frac, short_tol, index int32 (n,) or None)."""
    on_frac, short_tol = float(on_frac), float(short_tol)
    if math.isnan(on_frac) or on_frac < 0:
        raise ValueError(f"{who}: on_frac={on_frac} is negative or a NaN")
    if math.isnan(short_tol) or short_tol < 0:
        raise ValueError(f"{who}: short_tol={short_tol} is negative or a NaN")
    gid, G = check_pools(who, S, groups)
    return gid, G, on_frac, short_tol, check_index(who, n, index)


def check_tensor(who, what, p):
    """-> p (the `what`: "power", "profile") as (n, S, T)."""
    if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.dim() not in (2, 3):
        raise ValueError(f"{who}: the {what} must be a float32 tensor (residences, slots) or (residences, scenarios, slots)")
    if p.dim() == 2:
        p = p.unsqueeze(1)
    if p.numel() == 0 or p.stride(2) != 1:
        raise ValueError(f"{who}: the {what} is empty or its slots are not contiguous, {tuple(p.shape)}")
    return p


def check_on_device(who, p, homes, **choices):
    """What is left to check where the power lies on the device: every choice (rows=, nodes=) says read back, leave on
    the device or do not compute; p (n, S, T) lies on a GPU and homes holds its n S records there -> the device."""
    for name, value in choices.items():
        if value not in (True, False, "device"):
            raise ValueError(f'{who}: {name} must be True, False or "device", got {value!r}')
    n, S, _ = p.shape
    dev = p.device
    if dev.type != "cuda":
        raise ValueError(f"{who}: the power lies on {dev}; the report runs on the GPU")
    if not isinstance(homes, torch.Tensor) or homes.dtype != torch.uint8 or homes.numel() != n * S * HOME_DTYPE.itemsize \
            or not homes.is_contiguous() or homes.device != dev:
        raise ValueError(f"{who}: homes must hold {n * S} records of {HOME_DTYPE.itemsize} bytes (uint8, contiguous) on {dev}")
    return dev


def strides(p):
    """(stride_s, stride_i) of p (n, S, T); a dimension of one gets the stride that keeps the rows apart."""
    n, S, T = p.shape
    stride_i = p.stride(0) if n > 1 else S * max(p.stride(1), T)
    return p.stride(1) if S > 1 else n * stride_i, stride_i


def reorder(order, d_val, d_keep, d_row):
    """val (Q, S, n), keep (S, n) and the row records (S n record bytes, or None) with row i -> order[i], on the device."""
    if order is None:
        return d_val, d_keep, d_row
    S, n = d_keep.shape
    if d_row is not None:
        d_row = d_row.view(S, n, -1).index_select(1, order).contiguous().view(-1)
    return d_val.index_select(2, order), d_keep.index_select(1, order), d_row


def box_records(lib, stream, d_val, d_keep, d_index, gid, G):
    """The box records (Q, S) and their pools (Q, G), BILL_DTYPE, of val (Q, S, n) under keep (S, n): the selection the
    bill report has (revs_bill_study, no baseline: base = -1), once a quantity."""
    Q, S, n = d_val.shape
    rec = BILL_DTYPE.itemsize
    u8 = dict(dtype=torch.uint8, device=d_val.device)
    d_sum = torch.empty(Q, S, 2 * rec, **u8)
    d_pool = torch.empty(Q, G, 2 * rec, **u8) if G else None
    sel = torch.empty(int(lib.revs_bill_study_scratch(S, n)) // 8, dtype=torch.float64, device=d_val.device)
    h_base, h_group = np.full(S, -1, np.int32), np.ascontiguousarray(gid, np.int32)
    for q in range(Q):
        check(lib.revs_bill_study(S, n, ptr(d_val[q]), h_base.ctypes.data, ptr(d_keep), ptr(d_index),
                                  h_group.ctypes.data if G else None, G, None, ptr(d_sum[q]),
                                  ptr(d_pool[q]) if G else None, ptr(sel), stream), "revs_bill_study")
    box = d_sum.cpu().numpy().reshape(-1).view(BILL_DTYPE).reshape(Q, S, 2)[:, :, 0]
    pool = d_pool.cpu().numpy().reshape(-1).view(BILL_DTYPE).reshape(Q, G, 2)[:, :, 0] if G else np.zeros((Q, 0), BILL_DTYPE)
    return box, pool


def pooled_counts(slot, hist, gid, G, dtype):
    """(G, T) records of `dtype` (int64 fields of `slot`) and (G, planes, T + 1) int64: the members' counts added up."""
    pslot = np.zeros((G,) + slot.shape[1:], dtype)
    phist = np.zeros((G,) + hist.shape[1:], np.int64)
    for g in range(G):
        member = gid == g
        for k in dtype.names:
            pslot[k][g] = slot[k][member].astype(np.int64).sum(0)
        phist[g] = hist[member].astype(np.int64).sum(0)
    return pslot, phist


def host_rows(who, p, records):
    """A host caller's p (S, n, T) or (n, T) and records HOME_DTYPE (S, n) or (n,) -> (S, n, T, what is uploaded: p as
    float32 (n, S, T), the records' bytes [n][S])."""
    a, records = np.asarray(p), np.asarray(records)
    if a.ndim == 2:
        a = a[None]
    if records.ndim == 1:
        records = records[None]
    if a.ndim != 3 or a.size == 0:
        raise ValueError(f"{who}: p must be (residences, slots) or (scenarios, residences, slots), got {a.shape}")
    S, n, T = a.shape
    if records.dtype != HOME_DTYPE or records.shape != (S, n):
        raise ValueError(f"{who}: records must be HOME_DTYPE (scenarios, residences) = {(S, n)}, got {records.dtype} "
                         f"{records.shape}")
    h = np.ascontiguousarray(a.transpose(1, 0, 2), np.float32)
    return S, n, T, h, np.ascontiguousarray(records.T).view(np.uint8).reshape(-1)


def engine_sizes(who, engine, profile):
    """-> (S, n, T) of an engine (one scenario) or an ensemble (S), whose profile= names a policy where it is a string."""
    if isinstance(profile, str) and profile not in baselines.POLICIES:
        raise ValueError(f"{who}: profile must be None, one of {sorted(baselines.POLICIES)} or a tensor on the device, "
                         f"got {profile!r}")
    shape = engine._rule_shape()
    return shape[1] if len(shape) == 3 else 1, shape[0], shape[-1]


def engine_power(who, engine, profile, fill, charger):
    """The charger power a mixin reports on, in the engine's residence order: None, S of the last iteration (it raises
    unless that iteration wrote it); a policy name, the p of that rule schedule; a tensor of the engine's shape."""
    shape = engine._rule_shape()
    if profile is None:
        if engine._sc_iteration != engine.iteration:
            raise RuntimeError(f"{who}: the last iteration did not write the charger power (run_steps() and "
                               f"step(write_sc=False) leave it out): take one step(), or pass a profile")
        return engine.S.view(shape)
    if isinstance(profile, str):
        return baselines.rule_schedule_device(engine.homes, engine.load.view(engine.sweep_n, engine.sweep_T), profile, fill,
                                              charger, want="p", stream=engine.stream)[0].view(shape)
    if not isinstance(profile, torch.Tensor) or tuple(profile.shape) != tuple(shape) or profile.device != engine.S.device:
        raise ValueError(f"{who}: a power tensor must be {tuple(shape)} on {engine.S.device}, the engine's residence order")
    return profile
