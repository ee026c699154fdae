"""The power-flow report: the nonlinear branch-flow (DistFlow) equations of the radial feeder solved for every slot, next
to the linear model v^2 = vset^2 - R g that the scheduler and every other tree report read the feeder through -- true
node voltages, line flows and line losses, and cell by cell how far the linear voltages are off and which undervoltages
they miss.  Computed on the GPU by a fixed-point iteration over the network report's two scans (revs_net_powerflow:
include/revs_admm_ops.h).

One constant power factor for all loads; the reactances come per tree node as edge_x (None: active power only)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import PF_DAY_DTYPE, PF_NODE_DAY_DTYPE, PF_SLOT_DTYPE, check, ptr
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays


@dataclass
class PowerFlowReport:
    """volt / volt_lin: (nodes, T) float64 in the caller's node order, the branch-flow voltage and the linear model's;
    flow / loss: (nodes, T), kW through and lost on the line from tree node i to its parent; qflow: the same in kvar
    (None without edge_x) -- each None with arrays=False.  A slot that did not converge (slot["status"] != 0: 1 an
    injection that is not finite, 2 voltage collapse, 3 max_iter passes) reads NaN in every array but volt_lin.
    summary: (T,) SUMMARY_DTYPE, the box-plot record of the summarised nodes' voltages, n_violations = nodes below
    vmin, worst_value / worst_index = the lowest voltage and the lowest node that has it.  slot: (T,) PF_SLOT_DTYPE.
    node_day: (nodes,) PF_NODE_DAY_DTYPE.  day: one PF_DAY_DTYPE record."""
    volt: np.ndarray | None
    volt_lin: np.ndarray | None
    flow: np.ndarray | None
    loss: np.ndarray | None
    qflow: np.ndarray | None
    summary: np.ndarray
    slot: np.ndarray
    node_day: np.ndarray
    day: np.ndarray
    vset: float
    vmin: float
    slot_hours: float

    @property
    def error(self):
        """volt_lin - volt, (nodes, T): how far the linear model is above the branch-flow voltage."""
        if self.volt is None:
            raise ValueError("power-flow report: error needs the arrays (arrays=True)")
        return self.volt_lin - self.volt

    @property
    def converged(self) -> bool:
        """Whether every slot's iteration met tol."""
        return bool((self.slot["status"] == 0).all())

    def missed(self):
        """[(node, slot)] below vmin by the branch-flow voltage that the linear model passes."""
        if self.volt is None:
            raise ValueError("power-flow report: missed() needs the arrays (arrays=True)")
        with np.errstate(invalid="ignore"):
            at = (self.volt < self.vmin) & ~(self.volt_lin < self.vmin)
        return [(int(i), int(t)) for i, t in zip(*np.nonzero(at))]


def tan_phi_of(power_factor) -> float:
    """tan(acos(power_factor)) of a power factor in (0, 1]."""
    pf = float(power_factor)
    if not (0.0 < pf <= 1.0):
        raise ValueError(f"power-flow report: power_factor must lie in (0, 1], got {power_factor}")
    return math.tan(math.acos(pf))


def position_xw(dev, tree_host, n_nodes, edge_x):
    """xw = 2 x by preorder position (0 at padding positions), on the device; None -> None.  edge_x: one reactance per
    tree node, that of the line to its parent, laid out by tree["order"] exactly as feeder_tree lays out w."""
    if edge_x is None:
        return None
    x = np.asarray(edge_x, np.float64)
    if x.shape != (n_nodes,) or not np.isfinite(x).all():
        raise ValueError(f"power-flow report: edge_x must hold one finite reactance per tree node ({n_nodes})")
    order = np.asarray(tree_host["order"], np.int64)
    real = order < n_nodes
    return torch.from_numpy(np.ascontiguousarray(np.where(real, 2.0 * x[np.where(real, order, 0)], 0.0))).to(dev)


def native_powerflow_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, edge_x=None, power_factor=1.0, nodes=None,
                            vset=1.0, vmin=0.95, tol=1e-12, max_iter=32, cost=None, slot_hours=None, arrays=True) -> list:
    """revs_net_powerflow on node sums that lie on the device: node_g (S, M, T) float64 device tensor, tree: _lib.Tree,
    tree_host: the dict of feeder_tree, n_nodes: its nodes before padding -> S PowerFlowReports.  The one place the
    library is called from."""
    S, M, T = node_g.shape
    n = int(n_nodes)
    vset, vmin, tol, max_iter = float(vset), float(vmin), float(tol), int(max_iter)
    slot_hours = 24.0 / T if slot_hours is None else float(slot_hours)
    if not (np.isfinite(vset) and vset > 0.0):
        raise ValueError(f"power-flow report: vset must be finite and > 0, got {vset}")
    if not (np.isfinite(slot_hours) and slot_hours > 0.0):
        raise ValueError(f"power-flow report: slot_hours must be finite and > 0, got {slot_hours}")
    if not (np.isfinite(tol) and tol > 0.0):
        raise ValueError(f"power-flow report: tol must be finite and > 0, got {tol}")
    if not np.isfinite(vmin):
        raise ValueError(f"power-flow report: vmin must be finite, got {vmin}")
    if not 1 <= max_iter <= _lib.PF_MAX_ITER:
        raise ValueError(f"power-flow report: max_iter must lie in 1..{_lib.PF_MAX_ITER}, got {max_iter}")
    tan_phi = tan_phi_of(power_factor)
    d_xw = position_xw(dev, tree_host, n, edge_x)
    if d_xw is None:
        tan_phi = 0.0                          # (active power only: no reactance to carry a reactive flow over)
    d_nop, _, _ = side_arrays(dev, tree_host, n, None, None)
    d_nodes = tree_reports.position_mask(dev, tree_host, n, nodes, "no array", ("power-flow report", "nodes"))
    d_cost = None
    if cost is not None:
        if isinstance(cost, torch.Tensor):
            d_cost = cost.to(device=dev, dtype=torch.float64).contiguous()
        else:
            d_cost = torch.from_numpy(np.ascontiguousarray(cost, np.float64)).to(dev)
        if tuple(d_cost.shape) != (T,):
            raise ValueError(f"power-flow report: cost must have one entry per slot ({T}), got {tuple(d_cost.shape)}")
    d_arr = [None] * 5
    if arrays:
        d_arr = [torch.empty(S, n, T, dtype=torch.float64, device=dev) for _ in range(4)]
        d_arr.append(torch.empty(S, n, T, dtype=torch.float64, device=dev) if d_xw is not None else None)
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_slot = tree_reports.record_buffer(dev, PF_SLOT_DTYPE, S * T)
    d_nday = tree_reports.record_buffer(dev, PF_NODE_DAY_DTYPE, S * n)
    d_day = tree_reports.record_buffer(dev, PF_DAY_DTYPE, S)
    d_scratch = tree_reports.scratch("power-flow report", lib.revs_net_powerflow_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    check(lib.revs_net_powerflow(S, M, T, C.byref(tree), ptr(node_g), ptr(d_xw), tan_phi, ptr(d_nodes), ptr(d_nop), n,
                                 vset * vset, vmin, tol, max_iter, slot_hours, ptr(d_cost), *(ptr(d) for d in d_arr),
                                 ptr(d_sum), ptr(d_slot), ptr(d_nday), ptr(d_day), ptr(d_scratch), stream),
          "revs_net_powerflow")
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    slot = tree_reports.records(d_slot, PF_SLOT_DTYPE, S, T)
    nday = tree_reports.records(d_nday, PF_NODE_DAY_DTYPE, S, n)
    day = tree_reports.records(d_day, PF_DAY_DTYPE, S)
    host = [None if d is None else d.cpu().numpy() for d in d_arr]
    return [PowerFlowReport(*(None if h is None else h[s] for h in host), rec[s].copy(), slot[s].copy(), nday[s].copy(),
                            day[s].copy(), vset, vmin, slot_hours) for s in range(S)]


def powerflow_report_device(node_g, feeder=None, tree=None, edge_x=None, power_factor=1.0, nodes=None, vset=1.0, vmin=0.95,
                            tol=1e-12, max_iter=32, cost=None, slot_hours=None, arrays=True, lib=None, stream=None):
    """The power-flow report over node sums that lie on the device (shaped like losses.loss_report_device): node_g a
    contiguous float64 tensor, (S, M, T) -> a list of S PowerFlowReports, or (M, T) -> one; row cons_of[i] injected at
    tree node i.  The feeder comes as feeder=(parent, edge_r, cons_of) or as tree=(_lib.Tree, the dict of feeder_tree,
    nodes before padding).

    edge_x        per tree node, the reactance of the line to its parent (laid out as edge_r); None: active power only
    power_factor  one constant power factor for every load: q = tan(acos(power_factor)) p; read only with edge_x
    nodes         the tree nodes the summary, the extremes and the counts cover (indices or a boolean mask); None: all
    vset, vmin    the substation's voltage; the undervoltage limit the counts use
    tol, max_iter the iteration stops behind the pass whose largest |u_new - u_old| <= tol vset^2, or after max_iter
    cost          the tariff, one price per slot: day["cost"], the cost of the losses; None: NaN
    slot_hours    hours per slot; None: 24 / T
    arrays        False: the records only"""
    return tree_reports.device_report(
        "power-flow report", node_g, feeder, tree,
        lambda *on: native_powerflow_device(*on, edge_x, power_factor, nodes, vset, vmin, tol, max_iter, cost, slot_hours,
                                            arrays), lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, edge_x=None, power_factor=1.0, nodes=None, vset=1.0, vmin=0.95,
                    tol=1e-12, max_iter=32, cost=None, slot_hours=None, arrays=True, device="cuda:0"):
    """The power-flow report of node injections held on the host: node_p (M, T) or (S, M, T), row cons_of[i] injected
    at tree node i (network.report_for_tree's arguments) -> one PowerFlowReport or a list of S."""
    return tree_reports.host_report(device, (node_p,), lambda g: powerflow_report_device(
        g, feeder=(parent, edge_r, cons_of), edge_x=edge_x, power_factor=power_factor, nodes=nodes, vset=vset, vmin=vmin,
        tol=tol, max_iter=max_iter, cost=cost, slot_hours=slot_hours, arrays=arrays))


class PowerFlowMixin:
    def powerflow_report(self, profile=None, edge_x=None, power_factor=1.0, nodes=None, vmin=0.95, tol=1e-12, max_iter=32,
                         cost=None, slot_hours=None, arrays=True) -> PowerFlowReport:
        """The branch-flow voltages, flows and losses of a home profile beside the linear model's voltages
        (PowerFlowReport).  profile: as network_report's (None: the schedule's net load LOAD + P_sch).  cost: None, the
        engine's own tariff.  The other arguments: powerflow_report_device.  The voltage is the constructor's vset.
        With the residences sharded every rank returns the same report (the all-reduce of the node sums that
        network_report makes).  The run's state is read, never written."""
        if self._tree is None:
            raise ValueError("powerflow_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to "
                             "AdmmEngine")
        node_g = profile_node_sums(self, profile, "powerflow_report")
        if cost is None:
            cost = self.cost.to(torch.float64)
        return native_powerflow_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                       node_g[None], edge_x, power_factor, nodes, self.vset, vmin, tol, max_iter, cost,
                                       slot_hours, arrays)[0]
