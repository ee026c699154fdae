"""REVS fixture class with the reference's call surface (revs_fixture.py:60-280).

    fx = REVS(**file_params)
    tariff, homes, dist, save = fx.read_inputs(**inp_params)
    p, ev, soc = fx.get_distributed_optimal(tariff, homes, dist, save=True, **opt_params)

`get_distributed_optimal` and `get_individual_optimal` run on the MI355X engine;
the centralized MIQP and the plotting helpers are outside the hot path."""
from __future__ import annotations

import os

import numpy as np

from .extract import (GetCommunity, GetDistNet, GetHomeLoad, GetTariff, combine_result,
                      get_homes_ev_param)
from .lpsolver import (homes_to_arrays, solve_ADMM, solve_ADMM_many, solve_central, solve_residences,
                       solve_uncontrolled)

RULE_METHODS = ("uncontrolled", "last_minute", "trickle")       # baselines.POLICIES: REVS.study's rule methods


class REVS:
    def __init__(self, **kwargs):
        self.netID = kwargs.get("networkID", 121144)
        self.regID = kwargs.get("regionID", 121)
        self.com = kwargs.get("comunityID", 2)            # (sic) revs_fixture.py:64
        self.tariffID = kwargs.get("tariffID", "DVP")
        self.optim = kwargs.get("optimizer_mode", "individual")
        self.data_path = kwargs.get("data_path")
        out_path = kwargs.get("out_path")
        self.fig_dir = kwargs.get("fig_path")
        self.out_dir = f"{out_path}/{self.netID}-com{self.com}/{self.optim}"
        self.device = kwargs.get("device", "cuda:0")

    def _save(self, data, adopt, rating, seed):
        os.makedirs(self.out_dir, exist_ok=True)
        with open(f"{self.out_dir}/adopt{adopt}-rating{rating}-seed{seed}.txt", "w") as f:
            f.write(data)

    # ---- inputs (revs_fixture.py:114-189) ----
    def read_tariff(self, tariffID=None, shift=6):
        return GetTariff(self.data_path, tariffID or "DVP", shift)

    def read_homes(self, regionID=None, shift=6):
        return GetHomeLoad(self.data_path, regionID or self.regID, shift=shift)

    def read_network(self, networkID=None):
        return GetDistNet(self.data_path, networkID or self.netID)

    def read_community(self, networkID=None, com_index=2):
        return GetCommunity(f"{self.data_path}/{networkID or self.netID}-com.txt", com_index)

    def read_inputs(self, regionID=None, networkID=None, tariffID=None, ev_homes=None, **kwargs):
        adoption = kwargs.get("adoption", 90)
        rating = kwargs.get("rating", 4800)
        capacity = kwargs.get("capacity", 20)
        initial = kwargs.get("initial_soc", 0.2)
        start = kwargs.get("start_time", 11)
        end = kwargs.get("end_time", 23)
        sh = kwargs.get("shift_time", 6)
        seed = kwargs.get("seed", 1234)
        tariff = self.read_tariff(tariffID=tariffID, shift=sh)
        all_homes = self.read_homes(regionID=regionID, shift=sh)
        dist = self.read_network(networkID=networkID)
        com = self.read_community(networkID=networkID, com_index=self.com)
        if ev_homes is None or len(ev_homes) == 0:
            np.random.seed(int(seed))                      # revs_fixture.py:175-177
            ev_homes = np.random.choice(com, int(adoption * 1e-2 * len(com)), replace=False)
        homes = get_homes_ev_param(all_homes, dist, ev_homes, rating * 1e-3, capacity, initial,
                                   start, end)
        return tariff, homes, dist, dict(ev_homes=ev_homes, community=com)

    # ---- optimisation modes ----
    def get_individual_optimal(self, tariff, homes, save=False, **kwargs):
        """revs_fixture.py:192-222."""
        sol = solve_residences(tariff, homes, device=self.device)
        Pev = {h: sol[h][0] for h in homes}
        soc = {h: sol[h][1] for h in homes}
        Pres = {h: sol[h][2] for h in homes}
        if save:
            self._save(combine_result(Pres, Pev, soc, kwargs.get("ev_homes")),
                       kwargs.get("adoption", 90), kwargs.get("rating", 4800), kwargs.get("seed"))
        return Pres, Pev, soc

    def get_uncontrolled(self, tariff, homes, save=False, **kwargs):
        """The schedule nobody optimised (test-altered-profile.py:35-46: the charger runs from the arrival slot on)
        -> (Pres, Pev, soc) like get_individual_optimal.  **kwargs: policy ("uncontrolled" / "last_minute" / "trickle"),
        fill ("target" / "full"), charger ("binary" / "continuous") of lpsolver.solve_uncontrolled, and the labels
        `save` files the result under.  The tariff plays no part in a rule schedule; its length is the number of slots."""
        sol = solve_uncontrolled(homes, len(tariff), policy=kwargs.get("policy", "uncontrolled"),
                                 fill=kwargs.get("fill", "target"), charger=kwargs.get("charger", "binary"),
                                 device=self.device)
        Pev = {h: sol[h][0] for h in homes}
        soc = {h: sol[h][1] for h in homes}
        Pres = {h: sol[h][2] for h in homes}
        if save:
            self._save(combine_result(Pres, Pev, soc, kwargs.get("ev_homes")),
                       kwargs.get("adoption", 90), kwargs.get("rating", 4800), kwargs.get("seed"))
        return Pres, Pev, soc

    def get_centralized_optimal(self, tariff, homes, dist, save=False, **kwargs):
        """revs_fixture.py:225-249."""
        Pev, soc, Pres = solve_central(tariff, homes, dist, None, kwargs.get("v0", 1.03),
                                       kwargs.get("vmin", 0.90), kwargs.get("vmax", 1.05),
                                       device=self.device)
        if save:
            self._save(combine_result(Pres, Pev, soc, kwargs.get("ev_homes")),
                       kwargs.get("adoption", 90), kwargs.get("rating", 4800), kwargs.get("seed"))
        return Pres, Pev, soc

    def get_distributed_optimal(self, tariff, homes, dist, save=False, **kwargs):
        """revs_fixture.py:251-280; note the reference reads 'vlow'/'vhigh' (not
        'vmin'/'vmax') here, defaulting to 0.95 / 1.05.  return_engine=True: -> (Pres, Pev, soc, engine), the
        AdmmEngine that solved it (its multipliers: REVS.study(prices=...))."""
        diff, Pres, Pev, soc, *eng = solve_ADMM(
            homes, dist, tariff, None, kappa=kwargs.get("kappa", 5.0),
            iter_max=kwargs.get("max_iterations", 15), vset=kwargs.get("v0", 1.03),
            vlow=kwargs.get("vlow", 0.95), vhigh=kwargs.get("vhigh", 1.05),
            mode=kwargs.get("mode", "binary"), device=self.device, feeder=kwargs.get("feeder"),
            return_engine=bool(kwargs.get("return_engine", False)))
        if save:
            self._save(combine_result(Pres, Pev, soc, kwargs.get("ev_homes"), diff),
                       kwargs.get("adoption", 90), kwargs.get("rating", 4800), kwargs.get("seed"))
        return (Pres, Pev, soc) + tuple(eng)

    def study(self, tariff, all_homes, dist, community, adoptions, ratings, seeds,
              methods=("distributed", "individual"), group_by="method", ensemble=False, certify=False, device_report=False,
              across=False, bills=False, convergence=None, load_profile=False, charging=False, headroom=None, losses=False,
              transformers=False, flexibility=False, attribution=False, risk=False, prices=False, powerflow=False,
              **opt):
        """The grid of scenarios the reference's study scripts read back from disk (test-dist-ind-opt.py:219-342
        compare_method / compare_rating / compare_adoption, test-dist-ind-adopt.py:73-117 compare_node_counts), run
        and reported in one call -> (labels, study.StudyReport).

        For every adoption (%), rating (W) and seed -- in that nesting -- the EV homes are drawn from `community`
        exactly as read_inputs draws them, then every method of `methods` is solved; labels[s] = dict(method,
        adoption, rating, seed) of scenario s.  Methods: "distributed", "individual" and the rule schedules
        "uncontrolled", "last_minute", "trickle" (baselines.py; filled to opt rule_fill, "target" by default, for the
        charger of opt mode; labels[s]["unserved"] is then the number of residences whose EV leaves below the state of
        charge the model demands), labelled, grouped and pooled like any method.
        ONE study_report over all schedules' P_res follows, with
        nodes=community, the graph's line ratings, and pools by `group_by`: one label key or a tuple of them, a group
        being one distinct combination in order of first appearance ("method" at one adoption and rating:
        compare_method; "adoption" at one method: compare_adoption; "rating": compare_rating; ("method", "adoption"):
        every box of a grid).  StudyReport.band_counts / band_mean are compare_node_counts' bars.

        **opt: read_inputs' capacity, initial_soc, start_time, end_time; get_distributed_optimal's kappa,
        max_iterations, v0, vlow, vhigh, mode; the report's bands, vmin, vmax, arrays, report_vset (default 1.0, as
        drawing.compute_voltage) and line_rating ({line type: kVA}; default: the edges' `rating` attribute; without
        either the loading records are empty).  The feeder's matrix and tree are formed once.
        ensemble=True: the distributed scenarios of the grid are solved side by side (lpsolver.solve_ADMM_many, DESIGN.md
        section 3.9) instead of one engine after the other -- the same schedules to the operator's tolerance, not bit
        for bit.  certify=True (with ensemble=True): labels[s]["certificate"] of every distributed scenario is its
        engine.Certificate -- the schedule's cost, a dual bound below the centralized optimum and the gap between them,
        all scenarios of an ensemble certified together (AdmmEnsemble.certificates).  device_report=True (with
        ensemble=True): the distributed scenarios' rows of the report's input never leave the device -- every ensemble
        sums its schedules per row from its own state (solve_ADMM_many(return_node_sums=True)), the individual methods'
        profiles are uploaded as the float64 values they are, the (S, M, T) buffer is assembled on the device in label
        order and reported by study.study_report_device; labels, groups and every report field keep their meaning
        (StudyReport.node_p is the buffer read back).  across=True: StudyReport.across, per community node and per rated
        line the statistics across each group's scenarios (study.AcrossReport: in how many seeds a node goes below a
        band at some hour, its median daily minimum, the slots in violation) -- on either path from the arrays on the
        device.  bills=True: StudyReport.bills, the bills.BillReport of the study's rows (the residences) under
        `tariff`: every scenario's bills, their deviation from the schedule of method opt bill_base (default
        "individual") of the same (adoption, rating, seed) -- base[s] is that row, -1 without one -- and the records
        over each scenario's EV homes, pooled by the
        report's groups; on the device_report path from the buffer on the device.  convergence=eps (with ensemble=True):
        StudyReport.convergence, the convergence.ConvergenceReport of the distributed scenarios' residual histories at
        that eps, from the ensembles' histories on the device (solve_ADMM_many(return_convergence=eps)): its scenarios
        are the distributed ones in label order, `groups` their ids among the report's groups, pooled (G, iterations)
        by them -- a group without a distributed scenario has empty records.  load_profile=True:
        StudyReport.load_profile, the load_profile.LoadProfileReport of every method's schedules (the residences' rows),
        classes "without EV" / "with EV" by each scenario's own EV homes, pooled by the report's groups, followed by one
        row per (adoption, rating, seed) case with the base load "load" under that case's EV homes, in no pool
        (StudyReport.load_profile_rows names every row; opt profile_above: n_above's threshold, 0.0 by default).  The
        report works on float32, the precision of the engines' state; on the device_report path it reads the buffer on
        the device, otherwise the profiles are uploaded once.  charging=True: StudyReport.charging, the
        charging.ChargingReport of every method's charger power (the residences' rows, each scenario under its own
        records), pooled by the report's groups, costs under `tariff`; an ensemble's scenarios are read from the
        ensembles' own S on the device, the other methods' power is uploaded once as float32 (opt charging_on_frac,
        charging_short_tol: the report's thresholds, 0.0 and 1e-6 by default; the row records are read back with opt
        arrays).  headroom=need (kW): StudyReport.headroom, every scenario's headroom.HeadroomReport -- per node and
        slot the extra constant power that still fits under opt vmin and the line ratings, and what limits it -- over
        the nodes that carry residences, summarised over `community`, n_short against `need`; one launch for all
        scenarios, on the device_report path from the buffer on the device (its arrays are read back with opt
        arrays).  None: nothing of it runs.  losses=True or a dict of loss_report_device's options (lines, nodes,
        classes, slot_hours, loss_max, cost): StudyReport.losses, every scenario's losses.LossReport -- per line and
        slot the power lost, per node the marginal loss factor, the day's lost energy and its cost under `tariff` --
        summarised over every line unless lines= says otherwise; one launch for all scenarios on either path (its
        arrays are read back with opt arrays).  False: nothing of it runs.  transformers=True or a dict of
        transformer_report_device's options (xf_of, rated_kva, pf, ambient, model, slot_hours, substeps, initial,
        over_ratio, hot_limit): StudyReport.transformers, every scenario's transformers.TransformerReport -- per service
        transformer the load ratio, the top-oil and hot-spot temperatures and the day's loss of insulation life.  Without
        xf_of the owners come from the graph's labels (transformers.rows_by_transformer), without rated_kva the ratings
        from transformers.size_ratings of each transformer's base-load peak (at the dict's pf); one launch for all
        scenarios on either path (its arrays are read back with opt arrays).  False: nothing of it runs.
        flexibility=True: StudyReport.flexibility, the flexibility.FlexReport of every method's charger power -- per EV
        and slot how much charging could still be added or shed without the car leaving under target -- from the same
        buffer and records as charging=True, pooled by the report's groups, for the charger of opt mode (opt
        flexibility_on_frac, flexibility_short_tol: 0.0 and 1e-6 by default; the row records are read back with opt
        arrays; no node arrays: those are AdmmEngine.flexibility_report's, over the engine's nodes).
        attribution=True or a dict of attribution_report_device's options (watch, limit_nodes, classes, frac):
        StudyReport.attribution, every scenario's attribution.AttributionReport -- per slot the node of largest drop
        among those that carry residences, per node its contribution to that drop and the EVs' part of it -- from the
        report's own rows; the EV part is those rows minus the base load's, formed once in float64; counted and
        summarised over `community`, against opt vmin; one launch for all scenarios on either path (its arrays are read
        back with opt arrays).  False: nothing of it runs.
        risk=True or a dict of rel_sd (0.1), ev_rel_sd (0.0), common, p_max (0.05) and limit_nodes: StudyReport.risk, every
        scenario's risk.RiskReport -- per node and slot the odds of falling below opt vmin when the report's rows are a
        forecast: each residence's independent error has the standard deviation rel_sd x its base load + ev_rel_sd x its
        EV part (the row minus the base load), common lists up to two shared factors, ("load", c) / ("ev", c) or a
        loading array shaped like the rows; formed once in float64, counted and summarised over `community`; one launch
        for all scenarios on either path (its arrays are read back with opt arrays).  False: nothing of it runs.
        prices=True or a dict of price_report_device's options (scale, with_loss, lines, nodes, slot_hours, price_cap,
        cost): StudyReport.prices, every scenario's prices.PriceReport -- per node and slot the price (energy + marginal
        loss + congestion), per line the congestion rent -- from the report's own rows under the study's tariff and the
        multipliers of the scenario's voltage rows: those the operator holds after the last iteration of a
        "distributed" scenario (on either path), zero for every other method, whose schedules no voltage row shapes:
        their prices are energy and loss alone; against opt report_vset; one launch for all scenarios on either path
        (its arrays are read back with opt arrays).  False: nothing of it runs.
        powerflow=True or a dict of powerflow_report_device's options (edge_x, power_factor, nodes, vmin, tol, max_iter,
        slot_hours, cost): StudyReport.powerflow, every scenario's powerflow.PowerFlowReport -- the branch-flow voltages,
        flows and losses beside the linear model's voltages, and the undervoltages the linear model misses -- from the
        report's own rows; the reactances are read off the graph's edges where every edge carries an `x`
        (lpsolver.feeder_reactances; else active power only); counted and summarised over `community`, against opt vmin
        and opt report_vset; one launch for all scenarios on either path (its arrays are read back with opt arrays).
        False: nothing of it runs."""
        from .drawing import line_nodes
        from .lpsolver import feeder_of
        from . import study as st
        from .bills import bill_report, bill_report_device
        keys = (group_by,) if isinstance(group_by, str) else tuple(group_by)
        unknown = [k for k in keys if k not in ("method", "adoption", "rating", "seed")]
        unknown += [m for m in methods if m not in ("distributed", "individual") + RULE_METHODS]
        bill_base = opt.get("bill_base", "individual")
        if bill_base not in ("distributed", "individual") + RULE_METHODS:
            unknown.append(bill_base)
        if unknown:
            raise ValueError(f"REVS.study: unknown group key or method {unknown[0]!r}")
        if certify and not ensemble:
            raise ValueError("REVS.study: certify=True certifies the scenarios of an ensemble together: pass ensemble=True")
        if convergence is not None and not ensemble:
            raise ValueError("REVS.study: convergence=eps reports from the histories of an ensemble: pass ensemble=True")
        if device_report and not ensemble:
            raise ValueError("REVS.study: device_report=True reports from the state of an ensemble: pass ensemble=True")
        res = [n for n in dist if dist.nodes[n]["label"] == "H"]
        nonsub = [n for n in dist if dist.nodes[n]["label"] != "S"]
        pos = {n: i for i, n in enumerate(nonsub)}
        feeder = feeder_of(dist)
        parent, edge_r, cons_of = feeder[1]
        node_rating = None
        edges = list(dist.edges)
        if opt.get("line_rating") is not None or (edges and all("rating" in dist.edges[e] for e in edges)):
            node_rating = line_nodes(dist, opt.get("line_rating"), parent, nonsub)[0]
        # deferred: (position in profiles, homes) of the ensemble's scenarios; owners: every scenario's EV homes
        labels, profiles, deferred, owners = [], [], [], []
        want_p = bool(charging or flexibility)
        want_prices = prices is True or isinstance(prices, dict)
        mults = []                                 # prices: every scenario's row multipliers (None: zero)
        charge_p, charge_rec = [], []              # charging / flexibility: every scenario's charger power (None: deferred), records
        for adoption in adoptions:
            for rating in ratings:
                for seed in seeds:
                    np.random.seed(int(seed))                  # revs_fixture.py:175-177
                    ev_homes = np.random.choice(community, int(adoption * 1e-2 * len(community)), replace=False)
                    homes = get_homes_ev_param(all_homes, dist, ev_homes, rating * 1e-3, opt.get("capacity", 20),
                                               opt.get("initial_soc", 0.2), opt.get("start_time", 11),
                                               opt.get("end_time", 23))
                    for method in methods:
                        labels.append(dict(method=method, adoption=adoption, rating=rating, seed=seed))
                        owners.append(ev_homes)
                        mults.append(None)
                        if want_p:
                            charge_rec.append(homes_to_arrays(homes, res)[1])
                            charge_p.append(None)
                        if method == "distributed" and ensemble:
                            deferred.append((len(profiles), homes))
                            profiles.append(None)
                            continue
                        if method == "distributed" and want_prices:
                            from .prices import operator_multipliers
                            P_res, P_ev, _, eng = self.get_distributed_optimal(tariff, homes, dist, feeder=feeder,
                                                                               return_engine=True, **opt)
                            mults[-1] = operator_multipliers(eng, "operator", (eng.M, eng.T), "REVS.study").cpu().numpy()
                            del eng
                        elif method == "distributed":
                            P_res, P_ev = self.get_distributed_optimal(tariff, homes, dist, feeder=feeder, **opt)[:2]
                        elif method in RULE_METHODS:
                            sol, status = solve_uncontrolled(homes, len(tariff), policy=method,
                                                             fill=opt.get("rule_fill", "target"),
                                                             charger=opt.get("mode", "binary"), device=self.device,
                                                             return_status=True)
                            P_res, P_ev = {h: sol[h][2] for h in homes}, {h: sol[h][0] for h in homes}
                            labels[-1]["unserved"] = sum(1 for h in res if status[h] & 1)
                        else:
                            P_res, P_ev = self.get_individual_optimal(tariff, homes)[:2]
                        profiles.append(np.array([P_res[h] for h in res], np.float64))
                        if want_p:
                            charge_p[-1] = np.array([P_ev[h] for h in res], np.float32)
        conv_rep, charge_dev = None, None
        if deferred:
            sols = solve_ADMM_many([h for _, h in deferred], dist, tariff, None, kappa=opt.get("kappa", 5.0),
                                   iter_max=opt.get("max_iterations", 15), vset=opt.get("v0", 1.03),
                                   vlow=opt.get("vlow", 0.95), vhigh=opt.get("vhigh", 1.05),
                                   mode=opt.get("mode", "binary"), device=self.device, feeder=feeder,
                                   return_certificates=certify, return_node_sums=device_report,
                                   return_convergence=convergence,
                                   convergence_groups=self._deferred_groups(labels, keys, [i for i, _ in deferred]),
                                   convergence_patience=opt.get("patience", 8), return_charging=want_p,
                                   return_multipliers=want_prices)
            if want_prices:
                *head, mult_dev = sols
                sols = tuple(head) if len(head) > 1 else head[0]
                for k, (i, _) in enumerate(deferred):
                    mults[i] = mult_dev[k]
            if want_p:
                *head, charge_dev = sols
                sols = tuple(head) if len(head) > 1 else head[0]
            if convergence is not None:
                *head, conv_rep = sols
                sols = tuple(head) if len(head) > 1 else head[0]
            node_g = None
            if device_report:                    # (solutions[, certificates], node sums)
                *head, node_g = sols
                sols = tuple(head) if certify else head[0]
            if certify:
                sols, certs = sols
                for (i, _), cert in zip(deferred, certs):
                    labels[i]["certificate"] = cert
            for k, ((i, _), sol) in enumerate(zip(deferred, sols)):
                profiles[i] = node_g[k] if device_report else np.array([sol[1][h] for h in res], np.float64)
        combos = [tuple(lab[k] for k in keys) for lab in labels]
        order = list(dict.fromkeys(combos))
        bill_kw = None
        if bills:
            case = lambda lab: (lab["adoption"], lab["rating"], lab["seed"])
            ind = {case(lab): s for s, lab in enumerate(labels) if lab["method"] == bill_base}
            bill_kw = dict(base=[ind.get(case(lab), -1) for lab in labels], groups=[order.index(c) for c in combos],
                           keep=np.array([np.isin(res, ev) for ev in owners]), arrays=opt.get("arrays", False))
        prof_kw = None
        if load_profile:
            case = lambda lab: (lab["adoption"], lab["rating"], lab["seed"])
            cases = list(dict.fromkeys(case(lab) for lab in labels))
            first = [next(s for s, lab in enumerate(labels) if case(lab) == c) for c in cases]
            base_load = np.array([all_homes[h] for h in res], np.float32)
            prof_kw = dict(classes=np.array([np.isin(res, owners[s]) for s in list(range(len(labels))) + first], np.int64),
                           n_classes=2, names=("without EV", "with EV"), above=opt.get("profile_above", 0.0),
                           groups=[order.index(c) for c in combos] + [-1] * len(cases))
            prof_rows = [dict(lab) for lab in labels] + [dict(method="load", adoption=c[0], rating=c[1], seed=c[2])
                                                         for c in cases]

        def charger_power():
            import torch
            dev = torch.device(self.device)
            buf = torch.empty(len(res), len(labels), len(tariff), dtype=torch.float32, device=dev)
            where = {i: k for k, (i, _) in enumerate(deferred)}
            for s, p in enumerate(charge_p):
                buf[:, s].copy_(charge_dev[:, where[s]] if p is None else torch.from_numpy(p))
            rec = np.ascontiguousarray(np.stack(charge_rec, axis=1)).view(np.uint8).reshape(-1)
            return buf, torch.from_numpy(rec).to(dev)

        def charging_report():
            from .charging import charging_report_device
            return charging_report_device(*charger_power(), tariff,
                                          groups=[order.index(c) for c in combos],
                                          on_frac=opt.get("charging_on_frac", 0.0),
                                          short_tol=opt.get("charging_short_tol", 1e-6), rows=bool(opt.get("arrays", False)))

        def flexibility_report():
            from .baselines import CHARGERS
            from .flexibility import flexibility_report_device
            return flexibility_report_device(*charger_power(), CHARGERS[opt.get("mode", "binary")],
                                             groups=[order.index(c) for c in combos],
                                             on_frac=opt.get("flexibility_on_frac", 0.0),
                                             short_tol=opt.get("flexibility_short_tol", 1e-6),
                                             rows=bool(opt.get("arrays", False)), nodes=False)

        def headroom_reports(node_g):
            from .headroom import headroom_report_device
            return headroom_report_device(node_g, feeder=(parent, edge_r, cons_of), need=float(headroom), rating=node_rating,
                                          nodes=[pos[h] for h in community], vset=opt.get("report_vset", 1.0),
                                          vmin=opt.get("vmin", 0.95), arrays=opt.get("arrays", False))

        def loss_reports(node_g):
            from .losses import loss_report_device
            kw = dict(cost=np.asarray(tariff, np.float64))
            kw.update(losses if isinstance(losses, dict) else {})
            return loss_report_device(node_g, feeder=(parent, edge_r, cons_of), vset=opt.get("report_vset", 1.0),
                                      arrays=opt.get("arrays", False), **kw)

        def powerflow_reports(node_g):
            from .lpsolver import feeder_reactances
            from .powerflow import powerflow_report_device
            kw = dict(cost=np.asarray(tariff, np.float64), edge_x=feeder_reactances(dist, res),
                      nodes=[pos[h] for h in community], vmin=opt.get("vmin", 0.95))
            kw.update(powerflow if isinstance(powerflow, dict) else {})
            return powerflow_report_device(node_g, feeder=(parent, edge_r, cons_of), vset=opt.get("report_vset", 1.0),
                                           arrays=opt.get("arrays", False), **kw)

        def transformer_reports(node_g):
            from .transformers import rows_by_transformer, size_ratings, transformer_report_device
            kw = dict(transformers if isinstance(transformers, dict) else {})
            if "xf_of" not in kw:
                kw["xf_of"] = rows_by_transformer(dist, res)[1]
            if "rated_kva" not in kw:
                xf_of = np.asarray(kw["xf_of"], np.int64)
                base = np.zeros((int(xf_of.max(initial=-1)) + 1, len(tariff)))
                np.add.at(base, xf_of[xf_of >= 0], np.array([all_homes[h] for h in res], np.float64)[xf_of >= 0])
                kw["rated_kva"] = size_ratings(base.max(axis=1), pf=kw.get("pf", 0.95))
            return transformer_report_device(node_g, kw.pop("xf_of"), kw.pop("rated_kva"),
                                             arrays=opt.get("arrays", False), **kw)

        def attribution_reports(node_g):
            import torch
            from .attribution import attribution_report_device
            base = torch.from_numpy(np.array([all_homes[h] for h in res], np.float64)).to(node_g.device)
            kw = dict(nodes=[pos[h] for h in community])
            kw.update(attribution if isinstance(attribution, dict) else {})
            return attribution_report_device(node_g, (node_g - base[None]).contiguous(), feeder=(parent, edge_r, cons_of),
                                             vset=opt.get("report_vset", 1.0), vmin=opt.get("vmin", 0.95),
                                             arrays=opt.get("arrays", False), **kw)

        def risk_reports(node_g):
            import torch
            from .risk import common_spec, risk_report_device
            kw = dict(risk if isinstance(risk, dict) else {})
            base = torch.from_numpy(np.array([all_homes[h] for h in res], np.float64)).to(node_g.device)
            ev = node_g - base[None]
            sd = float(kw.pop("rel_sd", 0.1)) * base[None] + float(kw.pop("ev_rel_sd", 0.0)) * ev
            loads = []
            for it in common_spec("REVS.study", kw.pop("common", None)):
                if isinstance(it, tuple):
                    loads.append(float(it[1]) * (base[None].expand_as(node_g) if it[0] == "load" else ev))
                else:
                    loads.append(torch.as_tensor(np.asarray(it, np.float64), device=node_g.device).expand_as(node_g))
            kw.setdefault("nodes", [pos[h] for h in community])
            return risk_report_device(node_g, (sd * sd).contiguous(), torch.stack(loads).contiguous() if loads else None,
                                      feeder=(parent, edge_r, cons_of), vset=opt.get("report_vset", 1.0),
                                      vmin=opt.get("vmin", 0.95), arrays=opt.get("arrays", False), **kw)

        def price_reports(node_g):
            import torch
            from .prices import price_report_device
            kw = dict(cost=np.asarray(tariff, np.float64))
            kw.update(prices if isinstance(prices, dict) else {})
            node_y = torch.zeros_like(node_g)
            for s, y in enumerate(mults):
                if y is not None:
                    node_y[s].copy_(y if isinstance(y, torch.Tensor) else torch.from_numpy(y))
            return price_report_device(node_g, node_y, feeder=(parent, edge_r, cons_of), vset=opt.get("report_vset", 1.0),
                                       arrays=opt.get("arrays", False), **kw)
        want_xf = transformers is True or isinstance(transformers, dict)
        want_risk = risk is True or isinstance(risk, dict)
        want_attr = attribution is True or isinstance(attribution, dict)
        if device_report:
            import torch
            # (rows are residences here: the ensembles' node sums have one residence per row, like the profiles)
            buf = torch.empty(len(profiles), len(res), len(tariff), dtype=torch.float64, device=self.device)
            for s, prof in enumerate(profiles):
                buf[s].copy_(prof if isinstance(prof, torch.Tensor) else torch.from_numpy(prof))
            rep = st.study_report_device(buf, feeder=(parent, edge_r, cons_of), groups=[order.index(c) for c in combos],
                                         rating=node_rating, nodes=[pos[h] for h in community],
                                         bands=opt.get("bands", (0.92, 0.95, 0.98)), vset=opt.get("report_vset", 1.0),
                                         vmin=opt.get("vmin", 0.95), vmax=opt.get("vmax", 1.05),
                                         arrays=opt.get("arrays", False), across=across)
            if bills:
                rep.bills = bill_report_device(buf, tariff, **bill_kw)
            rep.convergence = conv_rep
            if load_profile:
                from .load_profile import load_profile_report_device
                d_load = torch.from_numpy(base_load).to(buf.device)
                g = torch.cat([buf.float(), d_load[None].expand(len(cases), -1, -1)]).permute(1, 0, 2).contiguous()
                rep.load_profile = load_profile_report_device(g, **prof_kw)
                rep.load_profile_rows = prof_rows
            if charging:
                rep.charging = charging_report()
            if headroom is not None:
                rep.headroom = headroom_reports(buf)
            if losses is True or isinstance(losses, dict):
                rep.losses = loss_reports(buf)
            if want_xf:
                rep.transformers = transformer_reports(buf)
            if flexibility:
                rep.flexibility = flexibility_report()
            if want_attr:
                rep.attribution = attribution_reports(buf)
            if want_risk:
                rep.risk = risk_reports(buf)
            if want_prices:
                rep.prices = price_reports(buf)
            if powerflow is True or isinstance(powerflow, dict):
                rep.powerflow = powerflow_reports(buf)
            return labels, rep
        rep = st.study_report(parent, edge_r, cons_of, np.stack(profiles), groups=[order.index(c) for c in combos],
                              rating=node_rating, nodes=[pos[h] for h in community],
                              bands=opt.get("bands", (0.92, 0.95, 0.98)), vset=opt.get("report_vset", 1.0),
                              vmin=opt.get("vmin", 0.95), vmax=opt.get("vmax", 1.05),
                              arrays=opt.get("arrays", False), device=self.device, across=across)
        if bills:
            rep.bills = bill_report(np.stack(profiles), tariff, device=self.device, **bill_kw)
        rep.convergence = conv_rep
        if load_profile:
            from .load_profile import load_profile_report
            g = np.concatenate([np.stack(profiles).astype(np.float32), np.broadcast_to(base_load, (len(cases),) + base_load.shape)])
            rep.load_profile = load_profile_report(g, device=self.device, **prof_kw)
            rep.load_profile_rows = prof_rows
        if charging:
            rep.charging = charging_report()
        if headroom is not None:
            import torch
            rep.headroom = headroom_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if losses is True or isinstance(losses, dict):
            import torch
            rep.losses = loss_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if want_xf:
            import torch
            rep.transformers = transformer_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if flexibility:
            rep.flexibility = flexibility_report()
        if want_attr:
            import torch
            rep.attribution = attribution_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if want_risk:
            import torch
            rep.risk = risk_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if want_prices:
            import torch
            rep.prices = price_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        if powerflow is True or isinstance(powerflow, dict):
            import torch
            rep.powerflow = powerflow_reports(torch.from_numpy(np.stack(profiles)).to(self.device))
        return labels, rep

    @staticmethod
    def _deferred_groups(labels, keys, which):
        """The study's group ids (distinct combinations of the label keys, in order of first appearance over ALL
        scenarios) of the scenarios `which`."""
        combos = [tuple(lab[k] for k in keys) for lab in labels]
        order = list(dict.fromkeys(combos))
        return [order.index(combos[i]) for i in which]

    def result_frames(self, demand, dist, community=None, start=11, end=23, shift=6, rating=None):
        """The two long tables the reference's box plots are drawn from (drawing.py:125-176, boxplot_flow /
        boxplot_volt), as dicts of numpy arrays: ({"hour", "loading"}, {"hour", "voltage"}) -- for every slot
        start..end the hour label and the loading in % of every edge of `dist`; the hour label and the voltage of
        every node of `community` (default: every non-substation node).  `rating`: see drawing.compute_flows."""
        from .drawing import compute_flows, compute_voltage
        flows = compute_flows(dist, demand, rating=rating, device=self.device)
        volts = compute_voltage(dist, demand, device=self.device)
        nodes = list(community) if community is not None else list(volts)
        slots = range(start, end + 1)
        label = {t: f"{(t + shift - 1) % 24}:00 - {(t + shift) % 24}:00" for t in slots}
        fl = {"hour": np.array([label[t] for t in slots for _ in flows]),
              "loading": np.array([abs(flows[e][t]) * 100.0 for t in slots for e in flows])}
        vo = {"hour": np.array([label[t] for t in slots for _ in nodes]),
              "voltage": np.array([volts[n][t] for t in slots for n in nodes])}
        return fl, vo

    def plot_result(self, *a, **k):
        """revs_fixture.py:282-...: figures (drawing.py: matplotlib / geopandas) are outside the hot
        path.  Warns and returns, so that a script written for the reference (test-optimizer.py:55-58
        computes everything, then plots) runs to its end."""
        import warnings
        warnings.warn("REVS.plot_result: plotting (drawing.py) is outside revs_admm_amd's scope; "
                      "nothing drawn", RuntimeWarning, stacklevel=2)
        return None
