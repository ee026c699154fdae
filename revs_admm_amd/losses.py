"""The loss report: how much power the feeder loses carrying a schedule, on which lines, in which slots, and what it
costs -- per line and slot the receiving-end branch-flow loss r P^2 / v on top of the network report's scans, per node
the marginal loss factor (the extra loss per extra kW drawn there), per slot and per day the sums over the feeder and
over classes of lines, the day's cost under a tariff and the eight lines that lose most.  Computed on the GPU
(revs_net_losses: include/revs_admm_ops.h).

The estimate is first-order, on a lossless flow model (the losses are not fed back into the flows), with active power
only; the marginal loss factor holds the voltages fixed."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import LOSS_DAY_DTYPE, LOSS_LINE_DAY_DTYPE, LOSS_SLOT_DTYPE, check, ptr
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays


@dataclass
class LossReport:
    """loss: (nodes, T) float64 in the caller's node order, kW lost on the line from tree node i to its parent in slot
    t; mlf: (nodes, T), the marginal loss factor of node i (dimensionless); flow / drop: (nodes, T), what they were
    computed from (the line flows and R p, the network report's bits) -- each None with arrays=False.  A bad slot (an
    injection that is not finite, or vset^2 - R p <= 0 at a node) reads NaN throughout.  summary: (T,) SUMMARY_DTYPE,
    the box-plot record of the summarised lines' losses, worst_value / worst_index = the largest loss and the lowest
    line that has it, n_violations = lines with loss > loss_max.  slot: (T,) LOSS_SLOT_DTYPE -- total, delivered,
    class_total, mlf_max, mlf_max_index, n_bad.  line_day: (nodes,) LOSS_LINE_DAY_DTYPE -- energy, peak, peak_slot.
    day: one LOSS_DAY_DTYPE record -- energy, delivered, class_energy, cost, peak, peak_slot, n_bad_slots, top_index /
    top_energy (the eight lines that lose most).  loss_percent: (T,) 100 total / delivered, formed on the host."""
    loss: np.ndarray | None
    mlf: np.ndarray | None
    summary: np.ndarray
    slot: np.ndarray
    line_day: np.ndarray
    day: np.ndarray
    loss_percent: np.ndarray
    vset: float
    slot_hours: float
    loss_max: float = float("inf")
    flow: np.ndarray | None = None
    drop: np.ndarray | None = None

    @property
    def day_loss_percent(self) -> float:
        """100 x the day's lost energy / the energy delivered."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(100.0 * self.day["energy"] / self.day["delivered"])

    @property
    def top_lines(self):
        """[(line, day energy)] of the up to eight summarised lines that lose most, descending."""
        return [(int(i), float(e)) for i, e in zip(self.day["top_index"], self.day["top_energy"]) if i >= 0]


def _position_bytes(dev, tree_host, n_nodes, sel, who):
    """tree_reports.position_mask of the loss report's lines= / nodes= (`who`); None: no array, every position."""
    return tree_reports.position_mask(dev, tree_host, n_nodes, sel, "no array", ("loss report", who))


def _position_classes(dev, tree_host, n_nodes, classes):
    """(uint8 per preorder position, C): the class of the line above the tree node there, 255 at padding positions and
    where classes[i] < 0; None -> (None, 0).  A class of LOSS_MAX_CLASSES or more is refused."""
    if classes is None:
        return None, 0
    cl = np.asarray(classes, np.int64)
    if cl.shape != (n_nodes,) or cl.max(initial=-1) >= _lib.LOSS_MAX_CLASSES:
        raise ValueError(f"loss report: classes must hold one class below {_lib.LOSS_MAX_CLASSES} (or -1) per tree node "
                         f"({n_nodes})")
    return tree_reports.position_classes(dev, tree_host, n_nodes, cl, _lib.LOSS_MAX_CLASSES)


def native_losses_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, lines=None, nodes=None, classes=None,
                         cost=None, slot_hours=None, loss_max=float("inf"), vset=1.0, arrays=True, out=None) -> list:
    """revs_net_losses on node sums that lie on the device: node_g (S, M, T) float64 device tensor, tree: _lib.Tree
    (device pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before padding -> S LossReports.  The one
    place the library is called from.  out: a contiguous (S, n_nodes, T) float64 device tensor that receives the losses
    and stays on the device (read back as well only with arrays=True)."""
    S, M, T = node_g.shape
    n = int(n_nodes)
    vset, loss_max = float(vset), float(loss_max)
    slot_hours = 24.0 / T if slot_hours is None else float(slot_hours)
    if not (np.isfinite(vset) and vset > 0.0):
        raise ValueError(f"loss report: vset must be finite and > 0, got {vset}")
    if not (np.isfinite(slot_hours) and slot_hours > 0.0):
        raise ValueError(f"loss report: slot_hours must be finite and > 0, got {slot_hours}")
    if not loss_max > 0.0:
        raise ValueError(f"loss report: loss_max must be > 0 (inf allowed), got {loss_max}")
    tree_reports.check_out("loss report", out, (S, n, T), node_g.device)
    d_nop, _, _ = side_arrays(dev, tree_host, n, None, None)
    d_lines = _position_bytes(dev, tree_host, n, lines, "lines")
    d_nodes = _position_bytes(dev, tree_host, n, nodes, "nodes")
    d_cls, n_cls = _position_classes(dev, tree_host, n, classes)
    d_cost = None
    if cost is not None:
        if isinstance(cost, torch.Tensor):
            d_cost = cost.to(device=dev, dtype=torch.float64).contiguous()
        else:
            d_cost = torch.from_numpy(np.ascontiguousarray(cost, np.float64)).to(dev)
        if tuple(d_cost.shape) != (T,):
            raise ValueError(f"loss report: cost must have one entry per slot ({T}), got {tuple(d_cost.shape)}")
    d_loss = out
    d_mlf = d_drop = d_flow = None
    if arrays:
        if d_loss is None:
            d_loss = torch.empty(S, n, T, dtype=torch.float64, device=dev)
        d_mlf, d_drop, d_flow = (torch.empty(S, n, T, dtype=torch.float64, device=dev) for _ in range(3))
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_slot = tree_reports.record_buffer(dev, LOSS_SLOT_DTYPE, S * T)
    d_lday = tree_reports.record_buffer(dev, LOSS_LINE_DAY_DTYPE, S * n)
    d_day = tree_reports.record_buffer(dev, LOSS_DAY_DTYPE, S)
    d_scratch = tree_reports.scratch("loss report", lib.revs_net_losses_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    check(lib.revs_net_losses(S, M, T, C.byref(tree), ptr(node_g), ptr(d_lines), ptr(d_nodes), ptr(d_cls), n_cls, ptr(d_nop),
                              n, vset * vset, slot_hours, loss_max, ptr(d_cost), ptr(d_loss), ptr(d_mlf), ptr(d_drop),
                              ptr(d_flow), ptr(d_sum), ptr(d_slot), ptr(d_lday), ptr(d_day), ptr(d_scratch), stream),
          "revs_net_losses")
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    slot = tree_reports.records(d_slot, LOSS_SLOT_DTYPE, S, T)
    lday = tree_reports.records(d_lday, LOSS_LINE_DAY_DTYPE, S, n)
    day = tree_reports.records(d_day, LOSS_DAY_DTYPE, S)
    if arrays:
        loss, mlf, drop, flow = (d.cpu().numpy() for d in (d_loss, d_mlf, d_drop, d_flow))
    reps = []
    for s in range(S):
        with np.errstate(divide="ignore", invalid="ignore"):
            pct = 100.0 * slot[s]["total"] / slot[s]["delivered"]
        reps.append(LossReport(loss[s] if arrays else None, mlf[s] if arrays else None, rec[s].copy(), slot[s].copy(),
                               lday[s].copy(), day[s].copy(), pct, vset, slot_hours, loss_max,
                               flow[s] if arrays else None, drop[s] if arrays else None))
    return reps


def loss_report_device(node_g, feeder=None, tree=None, lines=None, nodes=None, classes=None, cost=None, slot_hours=None,
                       loss_max=float("inf"), vset=1.0, arrays=True, out=None, lib=None, stream=None):
    """The loss report over node sums that lie on the device (shaped like headroom.headroom_report_device): node_g a
    contiguous float64 tensor, (S, M, T) -> a list of S LossReports, or (M, T) -> one; row cons_of[i] injected at tree
    node i.  The feeder comes as feeder=(parent, edge_r, cons_of) -- its tree is built and uploaded here, every row
    kept -- or as tree=(_lib.Tree, the dict of feeder_tree, nodes before padding) where it already lies on node_g's
    device (an engine's).

    lines         the tree nodes whose line to the parent the sums, the summary and the top 8 cover (indices or a
                  boolean mask); None: every line
    nodes         the tree nodes mlf_max looks at; None: every node
    classes       per tree node, the class 0..3 of the line to its parent (-1: in no class): class_total / class_energy
    cost          the tariff, one price per slot (array or tensor): day["cost"]; None: NaN
    slot_hours    hours per slot: energies are kW x slot_hours; None: 24 / T
    loss_max      kW: summary n_violations counts the lines that lose more
    vset          the substation's voltage: the losses divide by vset^2 - R p, formed here in double
    arrays        False: the records only
    out           a contiguous (S, tree nodes, T) float64 tensor on node_g's device that receives the losses and stays
                  there, e.g. for revs_net_across (study.native_across) across seeds with lo = -inf, hi = loss_max,
                  sense = +1"""
    return tree_reports.device_report(
        "loss report", node_g, feeder, tree,
        lambda *on: native_losses_device(*on, lines, nodes, classes, cost, slot_hours, loss_max, vset, arrays, out), lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, lines=None, nodes=None, classes=None, cost=None, slot_hours=None,
                    loss_max=float("inf"), vset=1.0, arrays=True, device="cuda:0"):
    """The loss report of node injections held on the host: node_p (M, T) or (S, M, T), row cons_of[i] injected at
    tree node i (network.report_for_tree's arguments) -> one LossReport or a list of S."""
    return tree_reports.host_report(device, (node_p,), lambda g: loss_report_device(
        g, feeder=(parent, edge_r, cons_of), lines=lines, nodes=nodes, classes=classes, cost=cost, slot_hours=slot_hours,
        loss_max=loss_max, vset=vset, arrays=arrays))


class LossMixin:
    def loss_report(self, profile=None, lines=None, nodes=None, classes=None, cost=None, slot_hours=None,
                    loss_max=float("inf"), arrays=True, out=None) -> LossReport:
        """What the feeder loses carrying a home profile: per line and slot the loss, per node the marginal loss factor,
        per slot and per day the sums, the cost and the lines that lose most (LossReport).

        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load,
                      (n, T) -- engine.rule_schedule("uncontrolled") or the base load go straight in
        lines, nodes, classes, loss_max   see loss_report_device
        cost          the tariff per slot; None: the engine's own
        slot_hours    None: 24 / T
        out           a (1, tree nodes, T) float64 device tensor for the losses (loss_report_device)

        The voltage is the constructor's vset.  With the residences sharded every rank returns the same report (the
        all-reduce of the node sums that network_report makes).  The run's state is read, never written."""
        if self._tree is None:
            raise ValueError("loss_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to AdmmEngine")
        node_g = profile_node_sums(self, profile, "loss_report")
        if cost is None:
            cost = self.cost.to(torch.float64)
        return native_losses_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                    node_g[None], lines, nodes, classes, cost, slot_hours, loss_max, self.vset, arrays,
                                    out)[0]
