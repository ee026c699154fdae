"""The network report: line flows, line loading and node voltages of a home profile, and their per-slot box-plot
numbers (what the reference draws for every result: drawing.py:29-78 compute_flows / compute_voltage, 125-176
boxplot_flow / boxplot_volt) -- computed on the GPU from the feeder as a tree (revs_net_node_sums, revs_net_report:
include/revs_admm_ops.h).  Drawing itself stays outside the project."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

# revs_net_summary_t (include/revs_admm_ops.h)
SUMMARY_DTYPE = np.dtype([("min", "<f8"), ("q1", "<f8"), ("median", "<f8"), ("q3", "<f8"), ("max", "<f8"),
                          ("whisker_lo", "<f8"), ("whisker_hi", "<f8"), ("worst_value", "<f8"), ("count", "<i4"),
                          ("n_fliers", "<i4"), ("n_violations", "<i4"), ("n_nan", "<i4"), ("worst_index", "<i4"),
                          ("reserved", "<i4", (3,))])
assert SUMMARY_DTYPE.itemsize == 96


@dataclass
class NetworkReport:
    """flow, loading, volt: (nodes, T) float64 in the caller's node order -- row i is tree node i and the line from
    i to its parent -- or None (arrays=False).  loading is NaN where the line has no rating; volt is NaN where
    vset^2 - R p < 0.  summary_loading / summary_volt: SUMMARY_DTYPE records, one per slot."""
    flow: np.ndarray | None
    loading: np.ndarray | None
    volt: np.ndarray | None
    summary_loading: np.ndarray
    summary_volt: np.ndarray
    node_sums: np.ndarray          # (M, T) float64: the profile summed over every node's residences
    vset: float
    vmin: float
    vmax: float

    @property
    def n_overloaded(self):
        """Lines with loading > 1, per slot."""
        return self.summary_loading["n_violations"].copy()

    @property
    def n_voltage_violations(self):
        """Nodes (of the summarised subset) outside [vmin, vmax], per slot."""
        return self.summary_volt["n_violations"].copy()

    @staticmethod
    def _worst(rec, key):
        ok = rec["count"] > 0
        if not ok.any():
            return None
        t = int(np.flatnonzero(ok)[np.argmax(key[ok])])          # (the earliest slot on ties)
        return int(rec["worst_index"][t]), t, float(rec["worst_value"][t])

    @property
    def worst_line(self):
        """(line, slot, loading) of the largest loading over all slots; None without a rated line."""
        return self._worst(self.summary_loading, self.summary_loading["worst_value"])

    @property
    def worst_node(self):
        """(node, slot, voltage) of the node farthest outside -- or nearest to the edge of -- [vmin, vmax]."""
        v = self.summary_volt["worst_value"]
        return self._worst(self.summary_volt, np.maximum(self.vmin - v, v - self.vmax))


def side_arrays(dev, tree_host, n_nodes, rating=None, nodes=None):
    """The per-position device arrays of revs_net_report / revs_net_study -> (node_of_pos, rating or None, mask or
    None): the caller's node index at every preorder position (-1: padding), the rating of the line above it (0:
    unrated) and whether the voltage summary covers it."""
    order = np.asarray(tree_host["order"], np.int64)
    real = order < n_nodes
    src = np.where(real, order, 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_nop = up(np.where(real, order, -1).astype(np.int32))
    d_rating = None
    if rating is not None:
        r = np.asarray(rating, np.float64)
        if r.shape != (n_nodes,):
            raise ValueError(f"network report: rating must have one entry per tree node ({n_nodes}), got {r.shape}")
        d_rating = up(np.where(real & (r[src] > 0), r[src], 0.0))
    d_mask = None
    if nodes is not None:
        mk = np.zeros(n_nodes, bool)
        mk[np.asarray(nodes)] = True
        d_mask = up((mk[src] & real).astype(np.uint8))
    return d_nop, d_rating, d_mask


def tree_on_device(dev, parent, edge_r, cons_of, n_rows):
    """feeder_tree of the whole feeder (every row kept) and its device form -> (tree_host, _lib.Tree, the tensors
    that back it: keep them alive)."""
    from .feeder import feeder_tree
    if len(parent) > _lib.TREE_MAX:
        raise ValueError(f"feeder has {len(parent)} nodes; the tree form holds {_lib.TREE_MAX}")
    th = feeder_tree(parent, edge_r, cons_of, np.ones(n_rows, bool))
    d_pack = torch.from_numpy(th["pack"].view(np.int64)).to(dev)
    d_w = torch.from_numpy(th["w"]).to(dev)
    return th, _lib.Tree(th["n"], ptr(d_pack), ptr(d_w)), (d_pack, d_w)


def run_report(lib, dev, stream, tree, tree_host, n_nodes, node_g, rating=None, nodes=None, vset=1.0, vmin=0.95,
               vmax=1.05, arrays=True) -> NetworkReport:
    """revs_net_report on node sums that lie on the device.  tree: _lib.Tree (device pack / w), tree_host: the dict of
    feeder_tree, n_nodes: its nodes before padding; node_g: (M, T) float64 device tensor; rating: per tree node (kVA of
    the line to its parent; NaN or <= 0: unrated) or None; nodes: indices or a boolean mask of the nodes the
    voltage summary covers (None: all)."""
    M, T = node_g.shape
    d_nop, d_rating, d_mask = side_arrays(dev, tree_host, n_nodes, rating, nodes)
    f64 = dict(dtype=torch.float64, device=dev)
    out = [torch.empty(n_nodes, T, **f64) for _ in range(3)] if arrays else [None] * 3
    d_sum = torch.zeros(2 * T * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    check(lib.revs_net_report(M, T, C.byref(tree), ptr(node_g), ptr(d_rating), ptr(d_mask), ptr(d_nop), n_nodes,
                              float(vset), float(vmin), float(vmax), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(d_sum),
                              stream), "revs_net_report")
    rec = d_sum.cpu().numpy().view(SUMMARY_DTYPE).reshape(2, T)
    flow, loading, volt = (None if o is None else o.cpu().numpy() for o in out)
    return NetworkReport(flow, loading, volt, rec[0].copy(), rec[1].copy(), node_g.cpu().numpy(), float(vset),
                         float(vmin), float(vmax))


def report_for_tree(parent, edge_r, cons_of, node_p, rating=None, nodes=None, vset=1.0, vmin=0.95, vmax=1.05,
                    arrays=True, device="cuda:0") -> NetworkReport:
    """The report of node injections held on the host: node_p (M, T), row cons_of[i] injected at tree node i.  (The
    engine's network_report sums the residences on the device instead.)"""
    from .engine import _dev_check
    lib, dev = _lib.load(), _dev_check(device)
    node_p = np.ascontiguousarray(node_p, np.float64)
    with torch.cuda.device(dev):
        th, tree, _keep = tree_on_device(dev, parent, edge_r, cons_of, node_p.shape[0])
        g = torch.from_numpy(node_p).to(dev)
        return run_report(lib, dev, torch.cuda.current_stream(dev).cuda_stream, tree, th, len(parent), g, rating,
                          nodes, vset, vmin, vmax, arrays)


def profile_node_sums(e, profile, who):
    """The (M, T) float64 node sums of a home profile of engine e on the device, all-reduced over the ranks: what
    network_report and headroom_report scan (profile: see network_report)."""
    if profile is None:
        load, prof = e.load, e.P_sch
    else:
        load = None
        if isinstance(profile, torch.Tensor):
            prof = profile
        else:
            prof = e._up(np.ascontiguousarray(np.asarray(profile, np.float32)[e.perm]))
        if prof.dtype != torch.float32 or tuple(prof.shape) != (e.n, e.T) or not prof.is_contiguous():
            raise ValueError(f"{who}: profile must be a contiguous float32 ({e.n}, {e.T}) array")
    node_g = torch.zeros(e.M, e.T, dtype=torch.float64, device=e.dev)
    if e.sweep_n:     # (node sums over node_ptr: load and profile read as n rows of T columns)
        check(e.lib.revs_net_node_sums(e.M, e.T, ptr(e.node_ptr), ptr(load), ptr(prof), ptr(node_g), e.stream),
              "revs_net_node_sums")
    e._allreduce(node_g)
    return node_g


class NetworkMixin:
    def network_report(self, profile=None, rating=None, nodes=None, arrays=True) -> NetworkReport:
        """Line flows, line loading and node voltages of a home profile over the whole feeder, per slot, and their
        per-slot summaries (NetworkReport).

        profile   None: the schedule's net load LOAD + P_sch.  Else the residences' net load itself, (n, T): a float32
                  tensor on the engine's device in the engine's residence order (like voltage()), or a numpy array in
                  the caller's order.
        rating    per tree node, the rating (kVA) of the line from that node to its parent; NaN or <= 0: unrated.
                  None: flows and voltages only -- loading is all NaN, its summary empty.
        nodes     indices (or a boolean mask) of the tree nodes the voltage summary covers; None: every node.
        arrays    False: the summaries only (the three (nodes, T) arrays are neither written nor copied).

        Tree nodes are those of feeder= (or of the tree recovered from Rn: engine.tree_recovered).  Voltages are
        sqrt(vset^2 - R p) with the constructor's vset; violations are counted against its vlow / vhigh.  With the
        residences sharded every rank returns the same report (one all-reduce of the M x T node sums).  The run's state
        (P_est, P_sch, G, the ring, the iteration count) is read, never written."""
        if self._tree is None:
            raise ValueError("network_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to "
                             "AdmmEngine (without it the engine recovers one from Rn only for the Newton operator "
                             "up to 4096 rows, and only when Rn is a radial feeder's matrix)")
        node_g = profile_node_sums(self, profile, "network_report")
        return run_report(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes, node_g,
                          rating, nodes, self.vset, self.vlow, self.vhigh, arrays)
