"""The price report: what the multipliers of the voltage rows say -- per node and slot the price a residence faces there
(energy + marginal loss + congestion: the distribution locational marginal price), per line the multiplier of the flow
through it, the congestion rent it collects and what an ohm less of it would save, per slot and per day who pays what
and the eight lines that collect most.  Computed on the GPU (revs_net_prices: include/revs_admm_ops.h, DESIGN.md
section 3.21).

The rows are the reference's vlow^2 - vset^2 <= R g <= vhigh^2 - vset^2 and y is signed in the operator's convention:
y > 0 where the upper row binds.  Load pulls R g up, so a binding upper row raises the price at every node whose path
to the substation shares a line with the row's node.  A run whose rows never bind has y = 0 and reports zero
congestion: that is the correct answer, not a missing one.

What the report does not say: the prices are those of the linearised (LinDistFlow) problem the scheduler solves, with
active power only; the marginal loss term holds the voltages fixed and is not part of the scheduler's objective; the
multipliers of an ADMM run that has not converged are not yet prices; and the reinforcement value is first order -- it
holds while the set of binding rows holds."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import LOSS_LINE_DAY_DTYPE, PRICE_DAY_DTYPE, PRICE_NODE_DAY_DTYPE, PRICE_SLOT_DTYPE, check, ptr
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays

WHO = "price report"


@dataclass
class PriceReport:
    """price, cong, lossp: (nodes, T) float64 in the caller's node order -- the nodal price and its congestion and
    marginal-loss parts (price = (cost + lossp) + cong); line_y, rent: (nodes, T), the multiplier Y of the flow through
    the line from tree node i to its parent and the rent s w Y flow that line collects; flow / drop: (nodes, T), the
    network report's bits -- each None with arrays=False.  A bad slot (an injection or a multiplier that is not finite,
    a scale that is not finite or negative, with the loss term vset^2 - R p <= 0 at a node) reads NaN in price, cong,
    lossp and rent.  summary: (T,) SUMMARY_DTYPE, the box-plot record of the summarised nodes' prices, worst_value /
    worst_index = the largest price and the lowest node that has it, n_violations = nodes with price > price_cap.
    slot: (T,) PRICE_SLOT_DTYPE.  node_day: (nodes,) PRICE_NODE_DAY_DTYPE -- paid, cong_paid, peak_price, peak_slot.
    line_day: (nodes,) LOSS_LINE_DAY_DTYPE on the rents -- energy = the day's rent.  day: one PRICE_DAY_DTYPE record."""
    price: np.ndarray | None
    cong: np.ndarray | None
    lossp: np.ndarray | None
    line_y: np.ndarray | None
    rent: np.ndarray | None
    drop: np.ndarray | None
    flow: np.ndarray | None
    summary: np.ndarray
    slot: np.ndarray
    node_day: np.ndarray
    line_day: np.ndarray
    day: np.ndarray
    scale: float
    vset: float
    slot_hours: float
    price_cap: float = float("inf")

    def reinforcement_value(self) -> np.ndarray:
        """(nodes, T): 2 s Y flow, the saving per hour per ohm taken off the line above the node (the envelope theorem:
        d optimum / d w_e = s Y_e P_e, and w = 2 r).  First order: it holds while the set of binding rows holds."""
        if self.line_y is None or self.flow is None:
            raise ValueError("reinforcement_value() needs the arrays: call the report with arrays=True")
        return 2.0 * self.scale * self.line_y * self.flow

    def shares(self) -> dict:
        """The energy, loss and congestion parts of the day's total payment in %."""
        e, l, c = (float(self.day[k]) for k in ("energy_pay", "loss_pay", "cong_pay"))
        tot = e + l + c
        with np.errstate(divide="ignore", invalid="ignore"):
            return {k: float(np.float64(100.0) * v / np.float64(tot)) for k, v in (("energy", e), ("loss", l), ("congestion", c))}

    @property
    def top_lines(self):
        """[(line, day rent)] of the up to eight summarised lines that collect most, descending."""
        return [(int(i), float(e)) for i, e in zip(self.day["top_index"], self.day["top_rent"]) if i >= 0]


def _f64_on(dev, name, a, shape):
    if a is None:
        return None
    t = a.to(device=dev, dtype=torch.float64).contiguous() if isinstance(a, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    if tuple(t.shape) != shape:
        raise ValueError(f"{WHO}: {name} must have shape {shape}, got {tuple(t.shape)}")
    return t


def scales_of(scale, S) -> np.ndarray:
    """scale= -> (S,) float64: a scalar for every scenario or one value each, finite and >= 0."""
    s = np.asarray(scale, np.float64)
    if s.ndim == 0:
        s = np.full(S, float(s))
    if s.shape != (S,) or not (np.isfinite(s) & (s >= 0.0)).all():
        raise ValueError(f"{WHO}: scale must be finite and >= 0, a scalar or one value per scenario ({S})")
    return s


def native_prices_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, node_y, scale=1.0, cost=None, with_loss=True,
                         lines=None, nodes=None, slot_hours=None, price_cap=float("inf"), vset=1.0, arrays=True) -> list:
    """revs_net_prices on node sums and multipliers that lie on the device: node_g, node_y (S, M, T) float64 device
    tensors, tree: _lib.Tree (device pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before padding
    -> S PriceReports.  The one place the library is called from."""
    S, M, T = node_g.shape
    n = int(n_nodes)
    vset, price_cap = float(vset), float(price_cap)
    slot_hours = 24.0 / T if slot_hours is None else float(slot_hours)
    if with_loss and not (np.isfinite(vset) and vset > 0.0):
        raise ValueError(f"{WHO}: vset must be finite and > 0, got {vset}")
    if not (np.isfinite(slot_hours) and slot_hours > 0.0):
        raise ValueError(f"{WHO}: slot_hours must be finite and > 0, got {slot_hours}")
    if price_cap != price_cap:
        raise ValueError(f"{WHO}: price_cap is a NaN")
    if cost is None:
        raise ValueError(f"{WHO}: cost is required, one price per slot")
    if (not isinstance(node_y, torch.Tensor) or node_y.dtype != torch.float64 or tuple(node_y.shape) != (S, M, T)
            or not node_y.is_contiguous() or node_y.device != node_g.device):
        raise ValueError(f"{WHO}: node_y must be a contiguous float64 {(S, M, T)} tensor on {node_g.device}")
    s_host = scales_of(scale, S)
    d_scale = torch.from_numpy(s_host).to(dev)
    d_cost = _f64_on(dev, "cost", cost, (T,))
    d_nop, _, _ = side_arrays(dev, tree_host, n, None, None)
    d_lines = tree_reports.position_mask(dev, tree_host, n, lines, "no array", (WHO, "lines"))
    d_nodes = tree_reports.position_mask(dev, tree_host, n, nodes, "no array", (WHO, "nodes"))
    f64 = dict(dtype=torch.float64, device=dev)
    d_arr = [torch.empty(S, n, T, **f64) for _ in range(7)] if arrays else [None] * 7
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_slot = tree_reports.record_buffer(dev, PRICE_SLOT_DTYPE, S * T)
    d_nday = tree_reports.record_buffer(dev, PRICE_NODE_DAY_DTYPE, S * n)
    d_lday = tree_reports.record_buffer(dev, LOSS_LINE_DAY_DTYPE, S * n)
    d_day = tree_reports.record_buffer(dev, PRICE_DAY_DTYPE, S)
    d_scratch = tree_reports.scratch(WHO, lib.revs_net_prices_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    check(lib.revs_net_prices(S, M, T, C.byref(tree), ptr(node_g), ptr(node_y), ptr(d_scale), ptr(d_cost), ptr(d_lines),
                              ptr(d_nodes), ptr(d_nop), n, vset * vset, 1 if with_loss else 0, slot_hours, price_cap,
                              *[ptr(d) for d in d_arr], ptr(d_sum), ptr(d_slot), ptr(d_nday), ptr(d_lday), ptr(d_day),
                              ptr(d_scratch), stream), "revs_net_prices")
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    slot = tree_reports.records(d_slot, PRICE_SLOT_DTYPE, S, T)
    nday = tree_reports.records(d_nday, PRICE_NODE_DAY_DTYPE, S, n)
    lday = tree_reports.records(d_lday, LOSS_LINE_DAY_DTYPE, S, n)
    day = tree_reports.records(d_day, PRICE_DAY_DTYPE, S)
    host = [None if d is None else d.cpu().numpy() for d in d_arr]
    return [PriceReport(*[None if a is None else a[s] for a in host], rec[s].copy(), slot[s].copy(), nday[s].copy(),
                        lday[s].copy(), day[s].copy(), float(s_host[s]), vset, slot_hours, price_cap) for s in range(S)]


def price_report_device(node_g, node_y, feeder=None, tree=None, scale=1.0, cost=None, with_loss=True, lines=None,
                        nodes=None, slot_hours=None, price_cap=float("inf"), vset=1.0, arrays=True, lib=None, stream=None):
    """The price report over node sums and row multipliers that lie on the device (shaped like
    losses.loss_report_device): node_g and node_y contiguous float64 tensors of one shape, (S, M, T) -> a list of S
    PriceReports, or (M, T) -> one; row cons_of[i] is injected at, and is the voltage row of, tree node i.  The feeder
    comes as feeder=(parent, edge_r, cons_of) or as tree=(_lib.Tree, the dict of feeder_tree, nodes before padding) where
    it already lies on node_g's device.

    node_y        the signed multipliers of the voltage rows, y > 0 where the upper row binds
    scale         s of L(s y): a scalar or one value per scenario, finite and >= 0 (Certificate.scale)
    cost          the tariff, one price per slot (array or tensor): required
    with_loss     False: no marginal loss term (lossp = 0; vset is then not used)
    lines         the tree nodes whose line to the parent rent_total and the top 8 cover; None: every line
    nodes         the tree nodes the summary, the payments and the extremes cover; None: every node
    slot_hours    hours per slot: payments are price x kW x slot_hours; None: 24 / T
    price_cap     summary n_violations counts the nodes whose price is above it
    vset          the substation's voltage: the loss term divides by vset^2 - R p, formed here in double
    arrays        False: the records only"""
    def native(*on):
        y3 = node_y[None] if node_g.dim() == 2 and isinstance(node_y, torch.Tensor) and node_y.dim() == 2 else node_y
        return native_prices_device(*on, y3, scale, cost, with_loss, lines, nodes, slot_hours, price_cap, vset, arrays)

    return tree_reports.device_report(WHO, node_g, feeder, tree, native, lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, node_y, scale=1.0, cost=None, with_loss=True, lines=None, nodes=None,
                    slot_hours=None, price_cap=float("inf"), vset=1.0, arrays=True, device="cuda:0"):
    """The price report of node injections and row multipliers held on the host: node_p, node_y (M, T) or (S, M, T), row
    cons_of[i] at tree node i (network.report_for_tree's arguments) -> one PriceReport or a list of S."""
    return tree_reports.host_report(device, (node_p, node_y), lambda g, y: price_report_device(
        g, y, feeder=(parent, edge_r, cons_of), scale=scale, cost=cost, with_loss=with_loss, lines=lines, nodes=nodes,
        slot_hours=slot_hours, price_cap=price_cap, vset=vset, arrays=arrays))


def operator_multipliers(e, multipliers, shape, who):
    """multipliers= of the engines' price reports -> a float64 tensor of `shape` in the operator's own layout, by
    certificate._bound_multipliers' rule: "operator" is the dual Newton path's current y, zero on the ADMM forms' path
    and when the last solve left no row with a multiplier; else an array of that shape."""
    if isinstance(multipliers, str):
        if multipliers != "operator":
            raise ValueError(f"{who}: multipliers is 'operator' or an array, not {multipliers!r}")
        use = e.op.solver == "newton" and e._y_support
        return e.yd[0].view(shape).clone() if use else torch.zeros(shape, dtype=torch.float64, device=e.dev)
    y = torch.as_tensor(np.asarray(multipliers, np.float64)).to(e.dev)
    if tuple(y.shape) != shape:
        raise ValueError(f"{who}: multipliers has shape {tuple(y.shape)}, expected {shape}")
    return y.contiguous()


class PriceMixin:
    def price_report(self, profile=None, multipliers="operator", scale=1.0, with_loss=True, lines=None, nodes=None,
                     cost=None, slot_hours=None, price_cap=float("inf"), arrays=True) -> PriceReport:
        """What the voltage limit costs and where: per node and slot the price (energy + marginal loss + congestion),
        per line the rent it collects and the value of reinforcing it, per slot and per day who pays what (PriceReport).

        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load
        multipliers   "operator": the dual Newton path's current row multipliers -- zero on the ADMM forms' path and
                      when the last solve left no row with a multiplier; else an (M, T) array, y > 0 at vhigh
        scale         s of L(s y), finite and >= 0; certificate().scale is the one that makes the bound tightest
        with_loss     False: no marginal loss term
        lines, nodes, price_cap   see price_report_device
        cost          the tariff per slot; None: the engine's own
        slot_hours    None: 24 / T

        A run whose rows never bind has y = 0 and reports zero congestion and zero rent on every line: that is the
        correct answer.  The voltage is the constructor's vset.  With the residences sharded every rank returns the same
        report: the node sums go through the all-reduce network_report makes, and y is every rank's own (the operator's
        state is the same on every rank).  The run's state is read, never written."""
        if self._tree is None:
            raise ValueError("price_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to AdmmEngine")
        y = operator_multipliers(self, multipliers, (self.M, self.T), "price_report")
        node_g = profile_node_sums(self, profile, "price_report")
        if cost is None:
            cost = self.cost.to(torch.float64)
        return native_prices_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                    node_g[None], y[None], scale, cost, with_loss, lines, nodes, slot_hours, price_cap,
                                    self.vset, arrays)[0]
