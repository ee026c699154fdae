"""The voltage attribution report: which nodes' load puts the watched node where it is, and how much of that is EV
charging -- per node and slot contrib[i] = R[j*][i] inj[i] for a watched node j* (a given one, or the slot's limit node of
largest drop), its EV part, the sums by class, the nodes that reach j*, carry a large share of its drop, or could clear
its excess alone.  A closed form on the feeder as a tree, computed on the GPU behind the network report's scans
(revs_net_attribution: include/revs_admm_ops.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import ATTR_DAY_DTYPE, ATTR_SLOT_DTYPE, check, ptr
from .headroom import aux_on_device, position_mask
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays


@dataclass
class AttributionReport:
    """sens / contrib / ev_contrib / drop: (nodes, T) float64 in the caller's node order, or None (arrays=False;
    ev_contrib also without node_ev) -- sens[i, t] = R[j*][i] for the slot's watched node j*, contrib = sens x the node's
    injection, ev_contrib = sens x its EV part, drop = R p (the network report's bits); NaN in a slot whose injections
    are not finite.  slot: (T,) ATTR_SLOT_DTYPE -- drop_watch, excess = max(0, drop_watch - drop_max), total, ev_total,
    class_total, the top 8 contributions and their nodes, watch (the tree node watched; -1: none), n_reach, n_big,
    n_can, n_bad.  summary: (T,) SUMMARY_DTYPE over the nodes that reach the watched one: the box-plot record of their
    contributions, n_violations = n_big, worst_value / worst_index = the largest contribution and the lowest node that
    has it, reserved[0] = nodes of `nodes` that do not reach it.  day: (nodes,) ATTR_DAY_DTYPE."""
    sens: np.ndarray | None
    contrib: np.ndarray | None
    ev_contrib: np.ndarray | None
    drop: np.ndarray | None
    slot: np.ndarray
    summary: np.ndarray
    day: np.ndarray
    frac: float
    vset: float
    vmin: float

    @property
    def drop_max(self):
        return self.vset * self.vset - self.vmin * self.vmin

    @property
    def watch(self):
        """The tree node watched in every slot; -1: none (no candidate, or a bad slot)."""
        return self.slot["watch"].copy()

    @property
    def ev_share(self):
        """ev_total / total per slot: the EVs' part of the watched node's drop (NaN where total is 0 or the slot bad)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.slot["total"] != 0.0, self.slot["ev_total"] / self.slot["total"], np.nan)

    def relief(self):
        """(nodes, T): the cut at node i alone that brings the slot's watched node back to vmin -- excess / sens where
        sens > 0, +inf where sens = 0 and excess > 0, 0 where excess = 0; NaN in a bad slot.  Formed here from sens and the
        slot records (one IEEE division, the one n_can counts with)."""
        if self.sens is None:
            raise ValueError("relief() needs the arrays: call the report with arrays=True")
        ex = self.slot["excess"][None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.sens > 0.0, ex / np.where(self.sens > 0.0, self.sens, 1.0), np.inf)
        r = np.where(ex == 0.0, 0.0, r)
        return np.where(np.isnan(ex) | np.isnan(self.sens), np.nan, r)


def class_array(dev, tree_host, n_nodes, classes):
    """classes: one integer 0..3 per tree node (anything else: no class) -> (uint8 per preorder position, C)."""
    cl = np.asarray(classes)
    if cl.shape != (n_nodes,):
        raise ValueError(f"attribution report: classes must have one entry per tree node ({n_nodes}), got {cl.shape}")
    return tree_reports.position_classes(dev, tree_host, n_nodes, cl, _lib.ATTR_MAX_CLASSES)


def native_attribution_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, node_ev=None, watch=None,
                              limit_nodes=None, nodes=None, classes=None, vset=1.0, vmin=0.95, frac=0.01,
                              arrays=True) -> list:
    """revs_net_attribution on node sums that lie on the device: node_g / node_ev (S, M, T) float64 device tensors, tree:
    _lib.Tree (device pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before padding -> S
    AttributionReports.  The one place the library is called from."""
    S, M, T = node_g.shape
    n = int(n_nodes)
    frac, vset, vmin = float(frac), float(vset), float(vmin)
    if not (np.isfinite(frac) and frac >= 0.0):
        raise ValueError(f"attribution report: frac must be finite and >= 0, got {frac}")
    if node_ev is not None and (not isinstance(node_ev, torch.Tensor) or node_ev.dtype != torch.float64
                                or tuple(node_ev.shape) != (S, M, T) or not node_ev.is_contiguous()
                                or node_ev.device != node_g.device):
        raise ValueError(f"attribution report: node_ev must be a contiguous float64 {(S, M, T)} tensor on {node_g.device}")
    watch_pos = -1
    if watch is not None:
        w = int(watch)
        if not 0 <= w < n:
            raise ValueError(f"attribution report: watch={w} is no tree node (0..{n - 1})")
        watch_pos = int(np.flatnonzero(np.asarray(tree_host["order"]) == w)[0])
    d_nop, _, _ = side_arrays(dev, tree_host, n, None, None)
    d_limit = None if limit_nodes is None else position_mask(dev, tree_host, n, limit_nodes)
    d_outm = position_mask(dev, tree_host, n, nodes)
    d_cls, n_cls = (None, 0) if classes is None else class_array(dev, tree_host, n, classes)
    aux, _keep = aux_on_device(dev, tree_host)
    f64 = dict(dtype=torch.float64, device=dev)
    d_sens = d_con = d_evc = d_drop = None
    if arrays:
        d_sens, d_con, d_drop = (torch.empty(S, n, T, **f64) for _ in range(3))
        if node_ev is not None:
            d_evc = torch.empty(S, n, T, **f64)
    d_slot = tree_reports.record_buffer(dev, ATTR_SLOT_DTYPE, S * T)
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_day = tree_reports.record_buffer(dev, ATTR_DAY_DTYPE, S * n)
    d_scratch = tree_reports.scratch("attribution report", lib.revs_net_attribution_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    drop_max = vset * vset - vmin * vmin
    check(lib.revs_net_attribution(S, M, T, C.byref(tree), C.byref(aux), ptr(node_g), ptr(node_ev), ptr(d_limit),
                                   ptr(d_outm), ptr(d_cls), n_cls, ptr(d_nop), n, watch_pos, drop_max, frac, ptr(d_sens),
                                   ptr(d_con), ptr(d_evc), ptr(d_drop), ptr(d_slot), ptr(d_sum), ptr(d_day),
                                   ptr(d_scratch), stream), "revs_net_attribution")
    slot = tree_reports.records(d_slot, ATTR_SLOT_DTYPE, S, T)
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    day = tree_reports.records(d_day, ATTR_DAY_DTYPE, S, n)
    host = [None if d is None else d.cpu().numpy() for d in (d_sens, d_con, d_evc, d_drop)]
    return [AttributionReport(*[None if a is None else a[s] for a in host], slot[s].copy(), rec[s].copy(), day[s].copy(),
                              frac, vset, vmin) for s in range(S)]


def attribution_report_device(node_g, node_ev=None, feeder=None, tree=None, watch=None, limit_nodes=None, nodes=None,
                              classes=None, vset=1.0, vmin=0.95, frac=0.01, arrays=True, lib=None, stream=None):
    """The attribution report over node sums that lie on the device (shaped like headroom.headroom_report_device): node_g
    a contiguous float64 tensor, (S, M, T) -> a list of S AttributionReports, or (M, T) -> one; row cons_of[i] injected
    at tree node i.  The feeder comes as feeder=(parent, edge_r, cons_of) or as tree=(_lib.Tree, the dict of feeder_tree,
    nodes before padding) where it already lies on node_g's device.

    node_ev       the EV part of node_g, shaped like it; None: ev_contrib is not computed, ev_total is +0.0, n_can 0
    watch         the tree node watched in every slot; None: per slot the limit node of largest drop
    limit_nodes   the tree nodes that can be watched (indices or a boolean mask); None: the nodes that carry a row
    nodes         the tree nodes the counts, the summary and the top 8 cover; None: the same nodes
    classes       one integer 0..3 per tree node (its lateral, zone, transformer group ...; anything else: no class):
                  class_total[k] sums the contributions of class k; None: no classes
    vset, vmin    the limit is a drop R p of vset^2 - vmin^2, formed here in double
    frac          n_big counts the nodes whose contribution exceeds frac x the watched node's drop
    arrays        False: the records only"""
    def native(*on):                # ((M, T) node sums come with (M, T) EV parts)
        ev3 = node_ev[None] if isinstance(node_ev, torch.Tensor) and node_g.dim() == 2 and node_ev.dim() == 2 else node_ev
        return native_attribution_device(*on, ev3, watch, limit_nodes, nodes, classes, vset, vmin, frac, arrays)

    return tree_reports.device_report("attribution report", node_g, feeder, tree, native, lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, node_ev=None, watch=None, limit_nodes=None, nodes=None, classes=None,
                    vset=1.0, vmin=0.95, frac=0.01, arrays=True, device="cuda:0"):
    """The attribution report of node injections held on the host: node_p (and node_ev, its EV part) (M, T) or (S, M, T),
    row cons_of[i] injected at tree node i -> one AttributionReport or a list of S."""
    return tree_reports.host_report(device, (node_p, node_ev), lambda g, ev: attribution_report_device(
        g, ev, feeder=(parent, edge_r, cons_of), watch=watch, limit_nodes=limit_nodes, nodes=nodes, classes=classes,
        vset=vset, vmin=vmin, frac=frac, arrays=arrays))


class AttributionMixin:
    def attribution_report(self, profile=None, ev_profile=None, watch=None, limit_nodes=None, nodes=None, classes=None,
                           frac=0.01, arrays=True) -> AttributionReport:
        """Which nodes' load causes the watched node's voltage drop in every slot, and how much of it is EV charging
        (AttributionReport).

        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load,
                      (n, T)
        ev_profile    the EV part of that profile, (n, T) like it; None: P_sch with the schedule, profile - LOAD (formed
                      in float32, the profile's own format) with a given profile
        watch         the tree node watched; None: per slot the limit node of largest drop
        limit_nodes   the tree nodes held at or above the constructor's vlow; None: the nodes that carry residences
        nodes         the tree nodes the counts and summaries cover; None: the same nodes
        classes       one integer 0..3 per tree node for class_total; None: no classes

        Voltage limits are those of the constructor (vset, vlow).  With the residences sharded every rank returns the
        same report (both node sums go through the all-reduce that network_report makes).  The run's state is read,
        never written."""
        if self._tree is None:
            raise ValueError("attribution_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to "
                             "AdmmEngine")
        who = "attribution_report"
        node_g = profile_node_sums(self, profile, who)
        if ev_profile is not None:
            node_ev = profile_node_sums(self, ev_profile, who)
        elif profile is None:
            node_ev = profile_node_sums(self, self.P_sch, who)
        else:
            prof = profile if isinstance(profile, torch.Tensor) else \
                self._up(np.ascontiguousarray(np.asarray(profile, np.float32)[self.perm]))
            node_ev = profile_node_sums(self, (prof - self.load).contiguous(), who)
        return native_attribution_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                         node_g[None], node_ev[None], watch, limit_nodes, nodes, classes, self.vset,
                                         self.vlow, frac, arrays)[0]
