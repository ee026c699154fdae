"""The headroom report: how much more charging the feeder can take, where, and when -- per node and slot the largest
extra constant power that node could draw before a limit node's voltage reaches vmin or a rated line on its path to the
substation reaches its rating, and which of the two stops it (the nodal hosting capacity; the question behind the
reference's adoption sweep, test-dist-ind-adopt.py:73-117).  A closed form on the feeder as a tree, computed on the GPU
behind the network report's scans (revs_net_headroom: include/revs_admm_ops.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import HEADROOM_DAY_DTYPE, check, ptr
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays
from .tree_reports import position_mask     # (dev, tree_host, n_nodes, nodes): None, the nodes that carry a row

KIND_VOLTAGE, KIND_THERMAL = 0, 1


@dataclass
class HeadroomReport:
    """headroom: (nodes, T) float64 in the caller's node order, kW of extra constant power node i could draw in slot t
    (+inf: nothing it affects is limited; 0: something is at or beyond its limit already; NaN: the slot's injections are
    not finite), or None (arrays=False).  limiter_node / limiter_kind: (nodes, T) int32, the tree node a and the kind of
    what stops the cell -- KIND_VOLTAGE (0): the subtree below a holds the limit node that reaches vmin first;
    KIND_THERMAL (1): the line above a; -1 / -1: unlimited.  summary: (T,) SUMMARY_DTYPE over the nodes of `nodes`: the
    box-plot record of the finite headrooms, n_violations = nodes with x < need, worst_value / worst_index = the smallest
    headroom and the lowest node that has it, reserved[0] = nodes with x = +inf.  day: (nodes,) HEADROOM_DAY_DTYPE -- the
    day's smallest headroom, its earliest slot, the slots with x < need.  drop / flow: (nodes, T), what the headrooms
    were computed from (R p and the line flows, the network report's bits), or None."""
    headroom: np.ndarray | None
    limiter_node: np.ndarray | None
    limiter_kind: np.ndarray | None
    summary: np.ndarray
    day: np.ndarray
    need: float
    vset: float
    vmin: float
    drop: np.ndarray | None = None
    flow: np.ndarray | None = None

    @property
    def n_short(self):
        """Nodes (of the summarised subset) where another charger of `need` kW does not fit, per slot."""
        return self.summary["n_violations"].copy()

    @property
    def fits(self):
        """Nodes with a finite headroom of at least `need`, per slot: count - n_violations (the unlimited ones are
        summary["reserved"][:, 0])."""
        return self.summary["count"] - self.summary["n_violations"]

    @property
    def tightest(self):
        """(node, slot, headroom) of the smallest headroom over all slots, the earliest slot on ties; None without a
        finite one."""
        ok = self.summary["count"] > 0
        if not ok.any():
            return None
        t = int(np.flatnonzero(ok)[np.argmin(self.summary["worst_value"][ok])])
        return int(self.summary["worst_index"][t]), t, float(self.summary["worst_value"][t])


def split_limiter(word):
    """limiter_out words -> (node, kind): node | kind << 30, -1: unlimited."""
    word = np.asarray(word, np.int32)
    none = word < 0
    return np.where(none, -1, word & 0x3FFFFFFF).astype(np.int32), np.where(none, -1, word >> 30).astype(np.int32)


def aux_on_device(dev, tree_host):
    """feeder.headroom_aux of a tree and its device form -> (_lib.HeadroomAux, the tensors that back it: keep them
    alive)."""
    from .feeder import headroom_aux
    ax = headroom_aux(tree_host)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_par, d_wc = up(ax["parent_pos"]), up(ax["wc"])
    d_jump = up(ax["jump"].view(np.int16)) if ax["n_jump"] else None
    return _lib.HeadroomAux(ptr(d_par), ptr(d_wc), ptr(d_jump), ax["n_jump"]), (d_par, d_wc, d_jump)


def native_headroom_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, need, rating=None, limit_nodes=None,
                           nodes=None, vset=1.0, vmin=0.95, arrays=True, out=None) -> list:
    """revs_net_headroom on node sums that lie on the device: node_g (S, M, T) float64 device tensor, tree: _lib.Tree
    (device pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before padding -> S HeadroomReports.  The
    one place the library is called from.  out: a contiguous (S, n_nodes, T) float64 device tensor that receives the
    headrooms and stays on the device (read back as well only with arrays=True)."""
    S, M, T = node_g.shape
    n = int(n_nodes)
    need, vset, vmin = float(need), float(vset), float(vmin)
    if not (np.isfinite(need) and need >= 0.0):
        raise ValueError(f"headroom report: need must be finite and >= 0, got {need}")
    tree_reports.check_out("headroom report", out, (S, n, T), node_g.device)
    d_nop, d_rating, _ = side_arrays(dev, tree_host, n, rating, None)
    d_limit = None if limit_nodes is None else position_mask(dev, tree_host, n, limit_nodes)
    d_outm = position_mask(dev, tree_host, n, nodes)
    aux, _keep = aux_on_device(dev, tree_host)
    d_head = out
    d_lim = d_drop = d_flow = None
    if arrays:
        if d_head is None:
            d_head = torch.empty(S, n, T, dtype=torch.float64, device=dev)
        d_lim = torch.empty(S, n, T, dtype=torch.int32, device=dev)
        d_drop, d_flow = (torch.empty(S, n, T, dtype=torch.float64, device=dev) for _ in range(2))
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_day = tree_reports.record_buffer(dev, HEADROOM_DAY_DTYPE, S * n)
    d_scratch = tree_reports.scratch("headroom report", lib.revs_net_headroom_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    drop_max = vset * vset - vmin * vmin
    check(lib.revs_net_headroom(S, M, T, C.byref(tree), C.byref(aux), ptr(node_g), ptr(d_rating), ptr(d_limit), ptr(d_outm),
                                ptr(d_nop), n, drop_max, need, ptr(d_head), ptr(d_lim), ptr(d_drop), ptr(d_flow), ptr(d_sum),
                                ptr(d_day), ptr(d_scratch), stream), "revs_net_headroom")
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    day = tree_reports.records(d_day, HEADROOM_DAY_DTYPE, S, n)
    reps = []
    if arrays:
        head, drop, flow = d_head.cpu().numpy(), d_drop.cpu().numpy(), d_flow.cpu().numpy()
        lnode, lkind = split_limiter(d_lim.cpu().numpy())
    for s in range(S):
        arr = (head[s], lnode[s], lkind[s]) if arrays else (None, None, None)
        reps.append(HeadroomReport(*arr, rec[s].copy(), day[s].copy(), need, vset, vmin,
                                   drop[s] if arrays else None, flow[s] if arrays else None))
    return reps


def headroom_report_device(node_g, feeder=None, tree=None, need=0.0, rating=None, limit_nodes=None, nodes=None, vset=1.0,
                           vmin=0.95, arrays=True, out=None, lib=None, stream=None):
    """The headroom report over node sums that lie on the device (shaped like study.study_report_device): node_g a
    contiguous float64 tensor, (S, M, T) -> a list of S HeadroomReports, or (M, T) -> one; row cons_of[i] injected at
    tree node i.  The feeder comes as feeder=(parent, edge_r, cons_of) -- its tree is built and uploaded here, every
    row kept -- or as tree=(_lib.Tree, the dict of feeder_tree, nodes before padding) where it already lies on node_g's
    device (an engine's).

    need          kW of the charger asked about: summary n_violations / day n_short count the cells with x < need
    rating        per tree node, the rating of the line to its parent in the unit of node_g; NaN or <= 0: unrated
    limit_nodes   the tree nodes whose voltage must stay at or above vmin (indices or a boolean mask); None: the nodes
                  that carry a row of node_g -- the rows the operator's QP holds (lpsolver.py:188-193)
    nodes         the tree nodes the summaries cover; None: the same nodes
    vset, vmin    the limit is a drop R p of vset^2 - vmin^2, formed here in double
    arrays        False: the summaries and the day records only
    out           a contiguous (S, tree nodes, T) float64 tensor on node_g's device that receives the headrooms and
                  stays there, e.g. for revs_net_across (study.native_across) across seeds: a cell with +inf members
                  gets numpy's NaN interpolation there."""
    return tree_reports.device_report(
        "headroom report", node_g, feeder, tree,
        lambda *on: native_headroom_device(*on, need, rating, limit_nodes, nodes, vset, vmin, arrays, out), lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, need=0.0, rating=None, limit_nodes=None, nodes=None, vset=1.0,
                    vmin=0.95, arrays=True, device="cuda:0"):
    """The headroom report of node injections held on the host: node_p (M, T) or (S, M, T), row cons_of[i] injected at
    tree node i (network.report_for_tree's arguments) -> one HeadroomReport or a list of S."""
    return tree_reports.host_report(device, (node_p,), lambda g: headroom_report_device(
        g, feeder=(parent, edge_r, cons_of), need=need, rating=rating, limit_nodes=limit_nodes, nodes=nodes, vset=vset,
        vmin=vmin, arrays=arrays))


def default_need(engine) -> float:
    """The largest charger rating among the engine's residence records with an EV (every rank's, when the residences
    are sharded); 0.0 without one."""
    rec = engine.homes.cpu().numpy().reshape(-1).view(_lib.HOME_DTYPE)
    ev = rec["ev"] != 0
    t = torch.tensor([float(rec["rating"][ev].max()) if ev.any() else 0.0], dtype=torch.float64, device=engine.dev)
    if engine.group is not None:
        engine._allreduce(t, op=torch.distributed.ReduceOp.MAX)
    return float(t.item())


class HeadroomMixin:
    def headroom_report(self, profile=None, need=None, rating=None, limit_nodes=None, nodes=None, arrays=True,
                        out=None) -> HeadroomReport:
        """How much more constant power every tree node could draw in every slot under a home profile, and what stops
        it (HeadroomReport).

        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load,
                      (n, T) -- engine.rule_schedule("uncontrolled") goes straight in
        need          kW of the charger asked about; None: the largest charger rating among the residence records
        rating        per tree node, the rating of the line to its parent; NaN or <= 0: unrated.  None: voltage alone
        limit_nodes   the tree nodes held at or above the constructor's vlow; None: the nodes that carry residences
        nodes         the tree nodes the summaries cover; None: the same nodes
        out           a (1, tree nodes, T) float64 device tensor for the headrooms (headroom_report_device)

        Voltage limits are those of the constructor (vset, vlow).  With the residences sharded every rank returns the
        same report (the all-reduce of the node sums that network_report makes).  The run's state is read, never
        written."""
        if self._tree is None:
            raise ValueError("headroom_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to AdmmEngine")
        node_g = profile_node_sums(self, profile, "headroom_report")
        if need is None:
            need = default_need(self)
        return native_headroom_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                      node_g[None], need, rating, limit_nodes, nodes, self.vset, self.vlow, arrays, out)[0]
