"""Rule-based charging baselines: the schedules nobody optimised.

    uncontrolled   the car charges from the first slot of its window on (test-altered-profile.py:35-46: the reference's
                   "before", constant charger power from the arrival slot laid over the base load)
    last_minute    it finishes in the last slot of its window
    trickle        the same power in every slot of its window (continuous chargers only)

each to the state of charge the model demands (fill="target": s_T >= 0.9) or to 100 % (fill="full").  The schedules follow
in closed form from the residence records (revs_rule_schedule, csrc/rule_kernels.hip); nothing here computes on the
host.  `rule_schedule` has the shape of engine.residence_solve; AdmmEngine.rule_schedule / AdmmEnsemble.rule_schedule
(the mixin below) run on the records and the load the sweep already holds and return the net load where
node_sums / study_report / voltages / network_reports(profile=...) take it."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import HOME_DTYPE, check, ptr

POLICIES = {"uncontrolled": _lib.RULE_ASAP, "last_minute": _lib.RULE_ALAP, "trickle": _lib.RULE_EVEN}
FILLS = {"target": _lib.FILL_TARGET, "full": _lib.FILL_FULL}
# charger: "binary" is the on/off charger; the engine's names of its continuous modes are accepted beside "continuous"
CHARGERS = {"binary": 1, "continuous": 0, "relaxed": 0, "pdhg": 0, "relaxed_exact": 0}


def rule_args(policy, fill, charger):
    """(policy, fill, integral) as revs_rule_schedule takes them; ValueError before anything is launched."""
    if policy not in POLICIES:
        raise ValueError(f"rule schedule: policy must be one of {sorted(POLICIES)}, got {policy!r}")
    if fill not in FILLS:
        raise ValueError(f"rule schedule: fill must be one of {sorted(FILLS)}, got {fill!r}")
    if isinstance(charger, str):
        if charger not in CHARGERS:
            raise ValueError(f"rule schedule: charger must be one of {sorted(CHARGERS)}, got {charger!r}")
        integral = CHARGERS[charger]
    else:                                          # (the engine's mode as a number)
        integral = 1 if int(charger) == _lib.MODE_BINARY else 0
    if policy == "trickle" and integral:
        raise ValueError('rule schedule: "trickle" needs a continuous charger (an on/off charger has no constant power '
                         'between 0 and its rating): pass charger="continuous"')
    return POLICIES[policy], FILLS[fill], integral


def rule_schedule_device(homes, load, policy="uncontrolled", fill="target", charger="binary", want="psgx", stream=None):
    """revs_rule_schedule over tensors on the device -> (p, soc, g, status) tensors; entries not in `want` are None.

    homes   uint8 (rows, 32) or (rows 32,): revs_home_t records (HOME_DTYPE bytes)
    load    float32 (rows, T), contiguous
    want    the outputs wanted, letters of "psgx": p (rows, T), soc (rows, T + 1), g = load + p (rows, T), status (rows,)
            int32 (bit 1: the EV leaves below the state of charge the model demands).  An output not wanted costs nothing."""
    pol, fil, integral = rule_args(policy, fill, charger)
    if not want or set(want) - set("psgx"):
        raise ValueError(f'rule schedule: want must be letters of "psgx", at least one, got {want!r}')
    if load.dtype != torch.float32 or load.dim() != 2 or not load.is_contiguous():
        raise ValueError("rule schedule: load must be a contiguous float32 (rows, T) tensor")
    rows, T = load.shape
    if homes.dtype != torch.uint8 or homes.numel() != rows * HOME_DTYPE.itemsize or not homes.is_contiguous():
        raise ValueError(f"rule schedule: homes must hold {rows} records of {HOME_DTYPE.itemsize} bytes (uint8, contiguous)")
    if homes.device != load.device:
        raise ValueError("rule schedule: homes and load live on different devices")
    lib, dev = _lib.load(), load.device
    f32 = dict(dtype=torch.float32, device=dev)
    p = torch.empty(rows, T, **f32) if "p" in want else None
    soc = torch.empty(rows, T + 1, **f32) if "s" in want else None
    g = torch.empty(rows, T, **f32) if "g" in want else None
    status = torch.empty(rows, dtype=torch.int32, device=dev) if "x" in want else None
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    check(lib.revs_rule_schedule(rows, T, ptr(homes), ptr(load), pol, fil, integral, ptr(p), ptr(soc), ptr(g), ptr(status),
                                 stream), "revs_rule_schedule")
    return p, soc, g, status


def rule_schedule(homes, load, policy="uncontrolled", fill="target", charger="binary", device="cuda:0"):
    """The rule schedule of every residence -> (p, soc, g, status) numpy arrays: charger power (n, T), state of charge
    (n, T + 1), net load g = load + p (n, T), status (n,) int32.  homes: HOME_DTYPE records (engine.pack_homes), load
    (n, T).  The shape of engine.residence_solve."""
    from .engine import _dev_check
    rule_args(policy, fill, charger)               # (before the device is touched)
    homes = np.ascontiguousarray(homes)
    load = np.ascontiguousarray(load, np.float32)
    if homes.dtype != HOME_DTYPE or load.ndim != 2 or homes.shape != (load.shape[0],):
        raise ValueError("rule schedule: homes must be one HOME_DTYPE record per row of the (n, T) load")
    _lib.load()
    dev = _dev_check(device)
    up = lambda a: torch.from_numpy(a).to(dev)
    out = rule_schedule_device(up(homes.view(np.uint8).reshape(-1, HOME_DTYPE.itemsize)), up(load), policy, fill, charger)
    return tuple(t.cpu().numpy() for t in out)


class RuleScheduleMixin:
    """AdmmEngine.rule_schedule (and, through it, AdmmEnsemble's)."""

    def rule_schedule(self, policy="uncontrolled", fill="target", charger=None) -> torch.Tensor:
        """The net load g = LOAD + p of a rule schedule on the records and the load the sweep holds (nothing is
        uploaded): a float32 tensor on the device in the engine's residence order, (n, T) -- an AdmmEnsemble's is
        (n, S, T) -- exactly what node_sums / study_report / voltages / network_reports(profile=...) accept.
        charger=None follows the engine's mode.  The run's state is read, never written."""
        g = rule_schedule_device(self.homes, self.load.view(self.sweep_n, self.sweep_T), policy, fill,
                                 self.mode if charger is None else charger, want="g", stream=self.stream)[2]
        return g.view(self._rule_shape())

    def _rule_shape(self):
        return (self.n, self.T)
