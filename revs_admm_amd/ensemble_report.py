"""Reports of an ensemble: every scenario's network report from the state on the device (revs_net_node_sums_many,
DESIGN.md sections 3.7 - 3.9).  What network.py and study.py do for schedules held on the host, for the S scenarios of
an AdmmEnsemble on the ensemble's own layout -- float[n][S][T], a residence's S T floats contiguous -- so no schedule
is read back, turned into dicts and uploaded again: ONE launch sums every scenario's residences per node straight into
revs_net_study's double[S][M][T], each scenario's slice bit for bit what revs_net_node_sums gives on that scenario
alone, and one revs_net_study reports on all of them.  Methods of AdmmEnsemble (mixed in by ensemble.py); nothing here
touches the run's state."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import study
from ._lib import check, ptr
from .network import NetworkReport, side_arrays


class EnsembleReportMixin:
    def _report_profile(self, profile):
        """The profile as a contiguous float32 tensor of n S T elements in the engine's residence order."""
        n, S, T = self.n_res, self.S_count, self.T_slot
        if profile is None:
            return self.P_sch
        if isinstance(profile, torch.Tensor):
            # (the three views the engine itself takes of a residence-side array)
            if (profile.dtype != torch.float32 or not profile.is_contiguous() or profile.device != self.P_sch.device
                    or tuple(profile.shape) not in ((n, S, T), (n * S, T), (n, S * T))):
                raise ValueError(f"node_sums: a profile on the device must be a contiguous float32 ({n}, {S}, {T}) tensor "
                                 f"on {self.dev} in the engine's residence order, got {tuple(profile.shape)} "
                                 f"{profile.dtype} on {profile.device}")
            return profile
        a = np.asarray(profile, np.float32)
        if a.shape != (S, n, T):
            raise ValueError(f"node_sums: a profile on the host must be (S, n, T) = {(S, n, T)} in the caller's "
                             f"residence order, got {a.shape}")
        return self._up(a.transpose(1, 0, 2)[self.perm])

    def node_sums(self, profile=None, add_load=False, out=None) -> torch.Tensor:
        """Every scenario's profile summed over each node's residences -> (S, M, T) float64 on the device, scenario s's
        slice bit for bit revs_net_node_sums on that scenario alone (one launch: revs_net_node_sums_many).

        profile   None: the schedules P_sch -- the residences' net load g = LOAD + p, what REVS.study reports.  Else a
                  contiguous float32 (n, S, T) tensor on the engine's device in the engine's residence order (the
                  layout of P_sch, S and load), or a numpy (S, n, T) array in the caller's order.
        add_load  True: the engine's LOAD is added to the profile, residence by residence before the sum -- for an
                  EV-only profile such as the charger powers S.
        out       where the sums go: a contiguous (S, M, T) float64 tensor on the device, e.g. the slice [s0:s0 + S] of
                  a larger study buffer; nothing outside it is written.  None: a new tensor."""
        S, M, T = self.S_count, self.M, self.T_slot
        prof = self._report_profile(profile)
        if out is None:
            out = torch.empty(S, M, T, dtype=torch.float64, device=self.dev)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (S, M, T)
              or not out.is_contiguous() or out.device != self.P_sch.device):
            raise ValueError(f"node_sums: out must be a contiguous float64 {(S, M, T)} tensor on {self.dev}")
        if not self.n_res:
            return out.zero_()
        check(self.lib.revs_net_node_sums_many(S, M, T, ptr(self.node_ptr), ptr(self.load) if add_load else None,
                                               ptr(prof), ptr(out), self.stream), "revs_net_node_sums_many")
        return out

    def _report_tree(self):
        if self._tree is None:
            raise ValueError("network_report needs the feeder as a tree: pass feeder=(parent, edge_r, cons_of) to "
                             "AdmmEngine (without it the engine recovers one from Rn only for the Newton operator "
                             "up to 4096 rows, and only when Rn is a radial feeder's matrix)")
        return self._tree, self._tree_host, self._tree_nodes

    def study_report(self, groups=None, rating=None, nodes=None, bands=(0.92, 0.95, 0.98), arrays=False, profile=None,
                     add_load=False, vset=None, vmin=None, vmax=None, across=False) -> study.StudyReport:
        """study.study_report of the S scenarios from the state on the device -> StudyReport: per-scenario summaries and
        band counts, box-plot numbers pooled over `groups`, with arrays=True flow / loading / volt of every scenario
        (groups, rating, nodes, bands, arrays: see study.study_report; tree nodes are those of feeder=, as
        AdmmEngine.network_report's).  profile / add_load: see node_sums -- the default reports P_sch alone.
        vset / vmin / vmax default to the constructor's vset / vlow / vhigh, as network_report's.  One node-sum launch
        and one revs_net_study; the records and StudyReport.node_p (S, M, T) are read back.  across=True (with groups):
        StudyReport.across, per node and per line the statistics across each group's scenarios, from the arrays on the
        device (study.across_report_device).  The run's state is read, never written."""
        study.check_across_groups(across, groups)
        bands, gid, _ = study.check_study_args(self.S_count, bands, groups)      # (before anything is launched)
        tree, tree_host, n_nodes = self._report_tree()
        node_g = self.node_sums(profile, add_load)
        return study.study_report_device(node_g, tree=(tree, tree_host, n_nodes), groups=None if groups is None else gid,
                                         rating=rating, nodes=nodes, bands=bands,
                                         vset=self.vset if vset is None else vset,
                                         vmin=self.vlow if vmin is None else vmin,
                                         vmax=self.vhigh if vmax is None else vmax, arrays=arrays, lib=self.lib,
                                         stream=self.stream, across=across)

    def voltages(self, profile=None, add_load=False, nodes=None, vset=None, out=None) -> torch.Tensor:
        """Every scenario's node voltages -> (S, nodes, T) float64 on the device, scenario s bit for bit
        network_reports()[s].volt: one node-sum launch and one revs_net_study with volt_out alone; nothing is read
        back.  profile / add_load: see node_sums; vset defaults to the constructor's.  nodes: None, every tree node of
        feeder= in its order; else the node indices wanted, gathered on the device.  out: a contiguous float64 tensor
        of the result's shape on the device to write into (with nodes=None the launch writes it directly)."""
        tree, tree_host, n_nodes = self._report_tree()
        S, T = self.S_count, self.T_slot
        idx = None if nodes is None else torch.as_tensor(np.asarray(nodes, np.int64), device=self.dev)
        shape = (S, n_nodes if idx is None else len(idx), T)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64
                                or tuple(out.shape) != shape or not out.is_contiguous()
                                or out.device != self.P_sch.device):
            raise ValueError(f"voltages: out must be a contiguous float64 {shape} tensor on {self.dev}")
        node_g = self.node_sums(profile, add_load)
        volt = out if out is not None and idx is None else torch.empty(S, n_nodes, T, dtype=torch.float64, device=self.dev)
        d_nop, _, _ = side_arrays(self.dev, tree_host, n_nodes)
        v = self.vset if vset is None else vset
        check(self.lib.revs_net_study(S, self.M, T, C.byref(tree), ptr(node_g), None, None, ptr(d_nop), n_nodes, float(v),
                                      float(self.vlow), float(self.vhigh), None, 0, None, 0, None, None, ptr(volt),
                                      None, None, None, None, self.stream), "revs_net_study")
        if idx is None:
            return volt
        picked = volt.index_select(1, idx)
        return picked if out is None else out.copy_(picked)

    def network_reports(self, rating=None, nodes=None, arrays=True, profile=None, add_load=False) -> list:
        """AdmmEngine.network_report for every scenario -> S NetworkReports, from study_report's single launch without
        pools and bands (revs_net_study gives every scenario the bits of revs_net_report on it alone)."""
        rep = self.study_report(None, rating, nodes, (), arrays, profile, add_load)
        pick = lambda a, s: None if a is None else a[s]
        return [NetworkReport(pick(rep.flow, s), pick(rep.loading, s), pick(rep.volt, s), rep.summary_loading[s],
                              rep.summary_volt[s], rep.node_p[s], rep.vset, rep.vmin, rep.vmax)
                for s in range(self.S_count)]

    def headroom_reports(self, need=None, rating=None, limit_nodes=None, nodes=None, arrays=True, profile=None,
                         add_load=False, out=None) -> list:
        """AdmmEngine.headroom_report for every scenario -> S headroom.HeadroomReports from one node-sum launch and one
        revs_net_headroom over all S (scenario s: the bits of the single engine's report on it).  need: None, the
        largest charger rating among all scenarios' records.  profile / add_load: see node_sums -- the default reports
        P_sch alone; out: a contiguous (S, tree nodes, T) float64 tensor on the device that receives the headrooms and
        stays there (revs_net_across takes it as it is).  The run's state is read, never written."""
        from . import headroom
        tree, tree_host, n_nodes = self._report_tree()
        if need is None:
            need = headroom.default_need(self)
        node_g = self.node_sums(profile, add_load)
        return headroom.native_headroom_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g, need,
                                               rating, limit_nodes, nodes, self.vset, self.vlow, arrays, out)

    def attribution_reports(self, watch=None, limit_nodes=None, nodes=None, classes=None, frac=0.01, arrays=True,
                            profile=None) -> list:
        """AdmmEngine.attribution_report for every scenario -> S attribution.AttributionReports from two node-sum
        launches and one revs_net_attribution over all S (scenario s: the bits of the single engine's report on it).
        profile: the EV part, see node_sums (None: the schedules P_sch); the injections are LOAD + profile.  The run's
        state is read, never written."""
        from . import attribution
        tree, tree_host, n_nodes = self._report_tree()
        node_g = self.node_sums(profile, True)
        node_ev = self.node_sums(profile, False)
        return attribution.native_attribution_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g,
                                                     node_ev, watch, limit_nodes, nodes, classes, self.vset, self.vlow,
                                                     frac, arrays)

    def risk_reports(self, rel_sd=0.1, ev_rel_sd=0.0, common=None, sd_profile=None, p_max=0.05, limit_nodes=None, nodes=None,
                     arrays=True, profile=None) -> list:
        """AdmmEngine.risk_report for every scenario -> S risk.RiskReports from 2 + K node-sum launches and one
        revs_net_risk over all S (scenario s: the bits of the single engine's report on it).  profile: the EV part, see
        node_sums (None: the schedules P_sch); the injections are LOAD + profile.  rel_sd, ev_rel_sd, sd_profile, common,
        p_max: as AdmmEngine.risk_report's, sd_profile and a loading profile in node_sums' forms.  The run's state is
        read, never written."""
        from . import risk
        tree, tree_host, n_nodes = self._report_tree()
        items = risk.common_spec("risk_reports", common)
        risk.z_of(p_max)                                         # (refused before anything is launched)
        ev = self._report_profile(profile)
        load = self.load.view(ev.shape)
        node_g = self.node_sums(ev, True)
        sd = self._report_profile(sd_profile) if sd_profile is not None else float(rel_sd) * load + float(ev_rel_sd) * ev
        node_var = self.node_sums((sd * sd).contiguous(), False)
        loads = []
        for it in items:
            if isinstance(it, tuple):
                it = (float(it[1]) * (load if it[0] == "load" else ev)).contiguous()
            loads.append(self.node_sums(it, False))
        node_common = torch.stack(loads).contiguous() if loads else None
        return risk.native_risk_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g, node_var,
                                       node_common, limit_nodes, nodes, self.vset, self.vlow, p_max, arrays)

    def loss_reports(self, lines=None, nodes=None, classes=None, cost=None, slot_hours=None, loss_max=float("inf"),
                     arrays=True, profile=None, add_load=False, out=None) -> list:
        """AdmmEngine.loss_report for every scenario -> S losses.LossReports from one node-sum launch and one
        revs_net_losses over all S (scenario s: the bits of the single engine's report on it).  cost: None, the
        ensemble's own tariff.  profile / add_load: see node_sums -- the default reports P_sch alone; out: a contiguous
        (S, tree nodes, T) float64 tensor on the device that receives the losses and stays there (revs_net_across takes
        it as it is).  The run's state is read, never written."""
        from . import losses
        tree, tree_host, n_nodes = self._report_tree()
        if cost is None:
            cost = self.cost.to(torch.float64)
        node_g = self.node_sums(profile, add_load)
        return losses.native_losses_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g, lines, nodes,
                                           classes, cost, slot_hours, loss_max, self.vset, arrays, out)

    def powerflow_reports(self, edge_x=None, power_factor=1.0, nodes=None, vmin=0.95, tol=1e-12, max_iter=32, cost=None,
                          slot_hours=None, arrays=True, profile=None) -> list:
        """AdmmEngine.powerflow_report for every scenario -> S powerflow.PowerFlowReports from one node-sum launch and one
        revs_net_powerflow over all S (scenario s: the bits of the single engine's report on it).  cost: None, the
        ensemble's own tariff.  profile: the EV part, see node_sums (None: the schedules P_sch); the injections are
        LOAD + profile.  The run's state is read, never written."""
        from . import powerflow
        tree, tree_host, n_nodes = self._report_tree()
        if cost is None:
            cost = self.cost.to(torch.float64)
        node_g = self.node_sums(profile, True)
        return powerflow.native_powerflow_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g, edge_x,
                                                 power_factor, nodes, self.vset, vmin, tol, max_iter, cost, slot_hours, arrays)

    def price_reports(self, multipliers="operator", scale=1.0, with_loss=True, lines=None, nodes=None, cost=None,
                      slot_hours=None, price_cap=float("inf"), arrays=True, profile=None) -> list:
        """AdmmEngine.price_report for every scenario -> S prices.PriceReports from one node-sum launch and one
        revs_net_prices over all S (scenario s: the bits of the single engine's report on it).  multipliers: "operator",
        the dual Newton path's current y -- yd[0] viewed (M, S, T) and brought to (S, M, T); zero on the ADMM forms' path
        and when the last solve left no row with a multiplier -- or an (S, M, T) array.  scale: a scalar or one value
        per scenario (certificates()[s].scale).  cost: None, the ensemble's own tariff.  profile: the EV part, see
        node_sums (None: the schedules P_sch); the injections are LOAD + profile.  The run's state is read, never
        written."""
        from . import prices
        tree, tree_host, n_nodes = self._report_tree()
        M, S, T = self.M, self.S_count, self.T_slot
        if isinstance(multipliers, str):
            y = prices.operator_multipliers(self, multipliers, (M, S, T), "price_reports").permute(1, 0, 2).contiguous()
        else:
            y = prices.operator_multipliers(self, multipliers, (S, M, T), "price_reports")
        prices.scales_of(scale, S)                               # (refused before anything is launched)
        if cost is None:
            cost = self.cost.to(torch.float64)
        node_g = self.node_sums(profile, True)
        return prices.native_prices_device(self.lib, self.dev, self.stream, tree, tree_host, n_nodes, node_g, y, scale, cost,
                                           with_loss, lines, nodes, slot_hours, price_cap, self.vset, arrays)

    def transformer_reports(self, xf_of, rated_kva, pf=0.95, ambient=30.0, model=None, slot_hours=None, substeps=1,
                            initial="cyclic", over_ratio=1.0, hot_limit=110.0, arrays=True, profile=None, add_load=False,
                            out=None) -> list:
        """AdmmEngine.transformer_report for every scenario -> S transformers.TransformerReports from one node-sum launch
        and one revs_xf_report over all S (scenario s: the bits of the single engine's report on it).  xf_of: per node
        row, the transformer it belongs to or -1; the rest as transformers.transformer_report_device.  profile /
        add_load: see node_sums -- the default reports P_sch alone; out: a contiguous (S, K, T) float64 tensor on the
        device that receives the hot-spots and stays there.  It needs no feeder tree.  The run's state is read, never
        written."""
        from . import transformers
        node_g = self.node_sums(profile, add_load)
        return transformers.transformer_report_device(node_g, xf_of, rated_kva, pf, ambient, model, slot_hours, substeps,
                                                      initial, over_ratio, hot_limit, arrays, out, lib=self.lib,
                                                      stream=self.stream)
