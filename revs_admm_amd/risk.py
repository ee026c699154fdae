"""The voltage risk report: how likely a schedule that clears vmin on paper is to fall below it -- the net load is a
forecast, with an independent error at every row and up to two shared factors (weather, "everybody comes home late"), and
the voltage drop is linear in it, so per node and slot the drop's standard deviation, its margin z in standard
deviations, the probability of undervoltage and the drop that is exceeded with probability p_max are a closed form on the
feeder as a tree, computed on the GPU with the network report's scans (revs_net_risk: include/revs_admm_ops.h, DESIGN.md
section 3.20)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from statistics import NormalDist

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import RISK_DAY_DTYPE, RISK_SLOT_DTYPE, check, ptr
from .headroom import aux_on_device, position_mask
from .network import SUMMARY_DTYPE, profile_node_sums, side_arrays


@dataclass
class RiskReport:
    """sd / z / prob / drop_q / drop: (nodes, T) float64 in the caller's node order, or None (arrays=False) -- sd the
    standard deviation of the node's drop, z = (drop_max - drop) / sd its margin (+-inf where sd = 0), prob = P(drop + error
    > drop_max) for Gaussian errors, drop_q = drop + z_max sd the drop that is exceeded with probability p_max, drop = R p
    (the network report's bits); NaN in a bad slot (a non-finite input or a negative variance).  slot: (T,)
    RISK_SLOT_DTYPE over the limit nodes among `nodes` -- expected (the sum of prob), n_risky (z < z_max), n_det (drop >
    drop_max), z_min / z_min_index / sd_at / drop_at, sd_max, n_bad.  summary: (T,) SUMMARY_DTYPE, the box-plot record of
    drop_q over the same nodes, n_violations = nodes with drop_q > drop_max, worst_value / worst_index = the largest
    drop_q and the lowest node that has it.  day: (nodes,) RISK_DAY_DTYPE over the slots that are not bad."""
    sd: np.ndarray | None
    z: np.ndarray | None
    prob: np.ndarray | None
    drop_q: np.ndarray | None
    drop: np.ndarray | None
    slot: np.ndarray
    summary: np.ndarray
    day: np.ndarray
    p_max: float
    z_max: float
    vset: float
    vmin: float

    @property
    def drop_max(self):
        return self.vset * self.vset - self.vmin * self.vmin

    def voltage_q(self, vset=None):
        """(nodes, T): sqrt(vset^2 - drop_q), the voltage every node stays above with probability 1 - p_max (NaN where
        the secure drop exceeds vset^2).  vset: None, the report's."""
        if self.drop_q is None:
            raise ValueError("voltage_q() needs the arrays: call the report with arrays=True")
        v = self.vset if vset is None else float(vset)
        x = v * v - self.drop_q
        with np.errstate(invalid="ignore"):
            return np.where(x < 0.0, np.nan, np.sqrt(np.where(x < 0.0, 0.0, x)))

    def prob_any(self):
        """(nodes,): 1 - prod over the slots of (1 - prob), the probability that the node is below the limit in at least
        one slot of the day -- formed here on the host, and ASSUMING INDEPENDENT SLOTS: forecast errors that persist
        from slot to slot make the true figure smaller (at least max over the slots of prob).  Bad slots are left out."""
        if self.prob is None:
            raise ValueError("prob_any() needs the arrays: call the report with arrays=True")
        return 1.0 - np.prod(np.where(np.isnan(self.prob), 1.0, 1.0 - self.prob), axis=1)


def z_of(p_max) -> float:
    """The standard deviations of margin that leave a probability p_max: the standard normal's quantile at 1 - p_max."""
    p = float(p_max)
    if not 0.0 < p <= 0.5:
        raise ValueError(f"risk report: p_max must lie in (0, 0.5], got {p}")
    return max(NormalDist().inv_cdf(1.0 - p), 0.0)


def _like(who, name, t, shape, dev):
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape
                          or not t.is_contiguous() or t.device != dev):
        raise ValueError(f"{who}: {name} must be a contiguous float64 {shape} tensor on {dev}")


def native_risk_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, node_var=None, node_common=None, limit_nodes=None,
                       nodes=None, vset=1.0, vmin=0.95, p_max=0.05, arrays=True) -> list:
    """revs_net_risk on node sums that lie on the device: node_g / node_var (S, M, T) and node_common (K, S, M, T) float64
    device tensors, tree: _lib.Tree (device pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before
    padding -> S RiskReports.  The one place the library is called from."""
    from .feeder import risk_weights
    S, M, T = node_g.shape
    n = int(n_nodes)
    vset, vmin = float(vset), float(vmin)
    z_max = z_of(p_max)
    _like("risk report", "node_var", node_var, (S, M, T), node_g.device)
    K = 0
    if node_common is not None:
        if not isinstance(node_common, torch.Tensor) or node_common.dim() != 4 or node_common.shape[0] > _lib.RISK_MAX_COMMON:
            raise ValueError(f"risk report: node_common must be a (K, {S}, {M}, {T}) tensor with K <= {_lib.RISK_MAX_COMMON}")
        K = int(node_common.shape[0])
    if K:
        _like("risk report", "node_common", node_common, (K, S, M, T), node_g.device)
    d_nop, _, _ = side_arrays(dev, tree_host, n, None, None)
    d_limit = None if limit_nodes is None else position_mask(dev, tree_host, n, limit_nodes)
    d_outm = position_mask(dev, tree_host, n, nodes)
    aux, _keep = aux_on_device(dev, tree_host)
    d_w2 = torch.from_numpy(np.ascontiguousarray(risk_weights(tree_host))).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    d_arr = [torch.empty(S, n, T, **f64) for _ in range(5)] if arrays else [None] * 5
    d_slot = tree_reports.record_buffer(dev, RISK_SLOT_DTYPE, S * T)
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_day = tree_reports.record_buffer(dev, RISK_DAY_DTYPE, S * n)
    d_scratch = tree_reports.scratch("risk report", lib.revs_net_risk_scratch(S, T, tree_host["n"]),
                                     f"S={S}, T={T}, tree of {tree_host['n']}", dev)
    drop_max = vset * vset - vmin * vmin
    check(lib.revs_net_risk(S, M, T, C.byref(tree), C.byref(aux), ptr(node_g), ptr(node_var), ptr(node_common) if K else None,
                            K, ptr(d_w2), ptr(d_limit), ptr(d_outm), ptr(d_nop), n, drop_max, z_max, *[ptr(d) for d in d_arr],
                            ptr(d_slot), ptr(d_sum), ptr(d_day), ptr(d_scratch), stream), "revs_net_risk")
    slot = tree_reports.records(d_slot, RISK_SLOT_DTYPE, S, T)
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, T)
    day = tree_reports.records(d_day, RISK_DAY_DTYPE, S, n)
    host = [None if d is None else d.cpu().numpy() for d in d_arr]
    return [RiskReport(*[None if a is None else a[s] for a in host], slot[s].copy(), rec[s].copy(), day[s].copy(),
                       float(p_max), z_max, vset, vmin) for s in range(S)]


def risk_report_device(node_g, node_var=None, node_common=None, feeder=None, tree=None, limit_nodes=None, nodes=None,
                       vset=1.0, vmin=0.95, p_max=0.05, arrays=True, lib=None, stream=None):
    """The risk report over node sums that lie on the device (shaped like headroom.headroom_report_device): node_g a
    contiguous float64 tensor, (S, M, T) -> a list of S RiskReports, or (M, T) -> one; row cons_of[i] injected at tree
    node i.  The feeder comes as feeder=(parent, edge_r, cons_of) or as tree=(_lib.Tree, the dict of feeder_tree, nodes
    before padding) where it already lies on node_g's device.

    node_var      the variance of the independent forecast error of every row, shaped like node_g (the variance of a
                  node's sum is the sum of its residences' variances); None: no independent error
    node_common   the loadings of up to two shared factors of unit variance, (K,) + node_g's shape: factor k moves row i
                  by node_common[k, ..., i, t] per standard deviation; None: no shared factor
    limit_nodes   the tree nodes whose voltage must stay at or above vmin (indices or a boolean mask); None: the nodes
                  that carry a row
    nodes         the tree nodes the slot records and the summary cover (among the limit nodes); None: the same nodes
    vset, vmin    the limit is a drop R p of vset^2 - vmin^2, formed here in double
    p_max         the probability of undervoltage a node may have, in (0, 0.5]: a node is at risk when z < z_max = the
                  standard normal's quantile at 1 - p_max
    arrays        False: the records only"""
    def native(*on):                # ((M, T) node sums come with (M, T) variances and (K, M, T) loadings)
        one = node_g.dim() == 2
        var3 = node_var[None] if one and isinstance(node_var, torch.Tensor) and node_var.dim() == 2 else node_var
        com4 = node_common[:, None] if one and isinstance(node_common, torch.Tensor) and node_common.dim() == 3 else node_common
        return native_risk_device(*on, var3, com4, limit_nodes, nodes, vset, vmin, p_max, arrays)

    return tree_reports.device_report("risk report", node_g, feeder, tree, native, lib, stream)


def report_for_tree(parent, edge_r, cons_of, node_p, node_var=None, node_common=None, limit_nodes=None, nodes=None, vset=1.0,
                    vmin=0.95, p_max=0.05, arrays=True, device="cuda:0"):
    """The risk report of node injections held on the host: node_p and node_var (M, T) or (S, M, T), node_common (K,) +
    that shape, row cons_of[i] injected at tree node i -> one RiskReport or a list of S."""
    return tree_reports.host_report(device, (node_p, node_var, node_common), lambda g, var, com: risk_report_device(
        g, var, com, feeder=(parent, edge_r, cons_of), limit_nodes=limit_nodes, nodes=nodes, vset=vset, vmin=vmin,
        p_max=p_max, arrays=arrays))


def common_spec(who, common):
    """common= of the engines' reports -> a list of up to two entries, each ("load" | "ev", coefficient) or a profile."""
    items = [] if common is None else list(common)
    if len(items) > _lib.RISK_MAX_COMMON:
        raise ValueError(f"{who}: at most {_lib.RISK_MAX_COMMON} shared factors, got {len(items)}")
    for it in items:
        if isinstance(it, str) or (isinstance(it, tuple) and (len(it) != 2 or it[0] not in ("load", "ev"))):
            raise ValueError(f'{who}: a shared factor is a profile or ("load" | "ev", coefficient), got {it!r}')
    return items


class RiskMixin:
    def risk_report(self, profile=None, rel_sd=0.1, ev_rel_sd=0.0, common=None, sd_profile=None, p_max=0.05,
                    limit_nodes=None, nodes=None, arrays=True) -> RiskReport:
        """How likely every node is to fall below the constructor's vlow in every slot when the home profile is a
        forecast (RiskReport).

        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load,
                      (n, T)
        rel_sd        the standard deviation of a residence's independent forecast error as a share of its base load
        ev_rel_sd     ... plus this share of its EV part (P_sch with the schedule, profile - LOAD with a given profile):
                      sd = rel_sd LOAD + ev_rel_sd EV, formed in float32, the profile's own format
        sd_profile    the residences' standard deviations themselves, (n, T) like a profile; then rel_sd and ev_rel_sd
                      are not used
        common        up to two shared factors of unit variance: each a loading profile (n, T) like a profile, or
                      ("load", c) / ("ev", c) for c x the base load / the EV part ("a day 5 % hotter than forecast":
                      ("load", 0.05))
        p_max         the probability of undervoltage a node may have, in (0, 0.5]
        limit_nodes   the tree nodes held at or above vlow; None: the nodes that carry residences
        nodes         the tree nodes the records cover; None: the same nodes

        The variance of a node's sum is the sum of its residences' variances: the squared standard deviations go through
        the node-sum launch of network_report, and so does every loading.  With the residences sharded every rank
        returns the same report (all of these sums go through the all-reduce network_report makes).  The run's state is
        read, never written."""
        if self._tree is None:
            raise ValueError("risk_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to AdmmEngine")
        who = "risk_report"
        items = common_spec(who, common)
        z_of(p_max)                                              # (refused before anything is launched)

        def as_dev(prof):
            return prof if isinstance(prof, torch.Tensor) else \
                self._up(np.ascontiguousarray(np.asarray(prof, np.float32)[self.perm]))

        ev = self.P_sch if profile is None else (as_dev(profile) - self.load)
        node_g = profile_node_sums(self, profile, who)
        sd = as_dev(sd_profile) if sd_profile is not None else float(rel_sd) * self.load + float(ev_rel_sd) * ev
        node_var = profile_node_sums(self, (sd * sd).contiguous(), who)
        loads = []
        for it in items:
            if isinstance(it, tuple):
                it = (float(it[1]) * (self.load if it[0] == "load" else ev)).contiguous()
            loads.append(profile_node_sums(self, it, who))
        node_common = torch.stack(loads)[:, None].contiguous() if loads else None
        return native_risk_device(self.lib, self.dev, self.stream, self._tree, self._tree_host, self._tree_nodes,
                                  node_g[None], node_var[None], node_common, limit_nodes, nodes, self.vset, self.vlow,
                                  p_max, arrays)[0]
