"""The study report: the network report of S schedules on one feeder in one pass on the GPU -- what the reference's
published figures are made of (test-dist-ind-opt.py:219-342 compare_method / compare_rating / compare_adoption: box
plots per hour pooled over all seeds of a group; test-dist-ind-adopt.py:73-117 compare_node_counts: per seed and hour
the number of residences at or below 0.92 / 0.95 / 0.98 p.u.).  revs_net_study (include/revs_admm_ops.h, DESIGN.md
section 3.8): per-schedule summaries and band counts from revs_net_report's kernel on a slots x schedules grid, and the
pooled box-plot numbers by an exact selection over the group's staged keys; revs_net_across: per node and per line the
statistics ACROSS the scenarios of a group (AcrossReport: which nodes fail, in how many seeds).  Drawing stays outside
the project."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import ACROSS_DTYPE, check, ptr
from .bills import check_scenarios
from .network import SUMMARY_DTYPE, side_arrays, tree_on_device

# revs_net_pooled_t (include/revs_admm_ops.h): revs_net_summary_t with worst_scenario in the first reserved word
POOLED_DTYPE = np.dtype([("min", "<f8"), ("q1", "<f8"), ("median", "<f8"), ("q3", "<f8"), ("max", "<f8"),
                         ("whisker_lo", "<f8"), ("whisker_hi", "<f8"), ("worst_value", "<f8"), ("count", "<i4"),
                         ("n_fliers", "<i4"), ("n_violations", "<i4"), ("n_nan", "<i4"), ("worst_index", "<i4"),
                         ("worst_scenario", "<i4"), ("reserved", "<i4", (2,))])
assert POOLED_DTYPE.itemsize == 96


@dataclass
class AcrossReport:
    """Statistics per node and per line across the scenarios of each group (revs_net_across):
    where the feeder fails and in how many scenarios.  ACROSS_DTYPE records -- min / q1 / median / q3 / max / mean over
    the group's scenarios, count, n_nan, n_violations, worst_scenario, band_count[b] -- of
    slot_volt / slot_loading     (G, nodes, T): the cell's values (None with slots=False)
    daily_volt / daily_loading   (G, nodes): every scenario's daily extreme, the lowest voltage / the highest loading of
                                 the day: band_count[b] is the number of scenarios in which the node goes at or below
                                 bands_volt[b] (the line reaches bands_loading[b]) at some hour
    exposure_volt / exposure_loading   (G, nodes) int32: the (scenario, slot) pairs in violation.
    The *_loading fields are None without line ratings.  Nodes outside `nodes` and unrated lines hold empty records
    (count 0).  group_sizes: (G,) scenarios per group."""
    slot_volt: np.ndarray | None
    slot_loading: np.ndarray | None
    daily_volt: np.ndarray
    daily_loading: np.ndarray | None
    exposure_volt: np.ndarray
    exposure_loading: np.ndarray | None
    group_sizes: np.ndarray
    bands_volt: tuple
    bands_loading: tuple

    def _kind(self, kind):
        if kind not in ("volt", "loading"):
            raise ValueError(f"across report: kind must be 'volt' or 'loading', got {kind!r}")
        daily, exposure = getattr(self, "daily_" + kind), getattr(self, "exposure_" + kind)
        if daily is None:
            raise ValueError("across report: no loading records (the report had no line ratings)")
        return daily, exposure

    def probability(self, kind, b):
        """(G, nodes): the share of the group's scenarios in which the node's daily extreme reaches band b --
        daily band_count[..., b] / count; NaN where count == 0."""
        daily, _ = self._kind(kind)
        cnt = daily["count"].astype(np.float64)
        return np.where(cnt > 0, daily["band_count"][..., b] / np.where(cnt > 0, cnt, 1.0), np.nan)

    def expected_slots(self, kind):
        """(G, nodes): the slots in violation per scenario -- exposure / count; NaN where count == 0."""
        daily, exposure = self._kind(kind)
        cnt = daily["count"].astype(np.float64)
        return np.where(cnt > 0, exposure / np.where(cnt > 0, cnt, 1.0), np.nan)


@dataclass
class StudyReport:
    """summary_loading / summary_volt: (S, T) SUMMARY_DTYPE records, scenario s's as report_for_tree gives them.
    pooled_loading / pooled_volt: (G, T) POOLED_DTYPE records over all values of a group's scenarios ((0, T) without
    groups).  band_counts: (S, T, B) int32, the nodes of `nodes` with volt <= bands[b] (cumulative; NaNs never
    counted).  flow, loading, volt: (S, nodes, T) float64 or None (arrays=False).  groups: (S,) int, -1: in no pool.
    node_p: (S, M, T) float64, the profiles reported.  across: the AcrossReport of across=True, else None.  bills: the
    bills.BillReport of REVS.study(bills=True), else None.  convergence: the convergence.ConvergenceReport of
    REVS.study(convergence=eps) over the ensemble's scenarios, else None.  load_profile: the
    load_profile.LoadProfileReport of REVS.study(load_profile=True), else None; its rows are load_profile_rows: the
    study's labels, then one row dict(method="load", adoption, rating, seed) per case -- the base load under that case's
    EV homes.  charging: the charging.ChargingReport of REVS.study(charging=True) over the study's scenarios, else
    None.  headroom / losses / transformers: every scenario's headroom.HeadroomReport / losses.LossReport /
    transformers.TransformerReport of REVS.study(headroom= / losses= / transformers=), else None.  flexibility: the
    flexibility.FlexReport of REVS.study(flexibility=True) over the study's scenarios, else None.  attribution: every
    scenario's attribution.AttributionReport of REVS.study(attribution=True), else None.  risk: every scenario's
    risk.RiskReport of REVS.study(risk=True), else None.  prices: every scenario's prices.PriceReport of
    REVS.study(prices=True), else None."""
    summary_loading: np.ndarray
    summary_volt: np.ndarray
    pooled_loading: np.ndarray
    pooled_volt: np.ndarray
    band_counts: np.ndarray
    bands: tuple
    groups: np.ndarray
    flow: np.ndarray | None
    loading: np.ndarray | None
    volt: np.ndarray | None
    node_p: np.ndarray
    vset: float
    vmin: float
    vmax: float
    across: AcrossReport | None = None
    bills: object | None = None
    convergence: object | None = None
    load_profile: object | None = None
    load_profile_rows: list | None = None
    charging: object | None = None
    headroom: list | None = None
    losses: list | None = None
    transformers: list | None = None
    flexibility: object | None = None
    attribution: list | None = None
    risk: list | None = None
    prices: list | None = None
    powerflow: list | None = None     # every scenario's powerflow.PowerFlowReport of REVS.study(powerflow=True), else None

    @property
    def n_groups(self):
        return len(self.pooled_volt)

    def band_mean(self):
        """(G, T, B): the mean of the band counts over each group's scenarios -- the height of the reference's bars
        (seaborn.barplot's estimator).  Its error bars are bootstrapped, i.e. random, and are not reproduced:
        band_range gives the spread instead.  NaN for a group without scenarios."""
        out = np.full((self.n_groups,) + self.band_counts.shape[1:], np.nan)
        for g in range(self.n_groups):
            if (self.groups == g).any():
                out[g] = self.band_counts[self.groups == g].mean(axis=0)
        return out

    def band_range(self):
        """((G, T, B), (G, T, B)): the smallest and the largest band count over each group's scenarios (-1 for a
        group without scenarios)."""
        lo = np.full((self.n_groups,) + self.band_counts.shape[1:], -1, np.int32)
        hi = lo.copy()
        for g in range(self.n_groups):
            if (self.groups == g).any():
                lo[g] = self.band_counts[self.groups == g].min(axis=0)
                hi[g] = self.band_counts[self.groups == g].max(axis=0)
        return lo, hi


def native_across(lib, stream, values, keep, groups, n_groups, lo, hi, sense, bands, slots):
    """revs_net_across on values that lie on the device: values (S, n, T) float64 device tensor, keep (n,) bool or None,
    groups (S,) int32 in -1 .. n_groups - 1 -> (slot records (G, n, T) or None, daily records (G, n), exposure (G, n)
    int32), read back.  The one place this entry is called from (a host test puts tests/across_ref.py here)."""
    S, n, T = values.shape
    dev, G, B = values.device, int(n_groups), len(bands)
    rec = ACROSS_DTYPE.itemsize
    d_keep = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)
    d_slot = torch.empty(G * n * T * rec, dtype=torch.uint8, device=dev) if slots else None
    d_daily = torch.empty(G * n * rec, dtype=torch.uint8, device=dev)
    d_exp = torch.empty(G, n, dtype=torch.int32, device=dev)
    d_scratch = tree_reports.scratch("across report", lib.revs_net_across_scratch(S, n), f"S={S}, {n} nodes", dev)
    h_group = np.ascontiguousarray(groups, np.int32)
    h_band = np.ascontiguousarray(bands, np.float64)
    check(lib.revs_net_across(S, n, T, ptr(values), ptr(d_keep), h_group.ctypes.data, G, float(lo), float(hi), int(sense),
                              h_band.ctypes.data if B else None, B, ptr(d_slot), ptr(d_daily), ptr(d_exp),
                              ptr(d_scratch), stream), "revs_net_across")
    slot = tree_reports.records(d_slot, ACROSS_DTYPE, G, n, T) if slots else None
    return slot, tree_reports.records(d_daily, ACROSS_DTYPE, G, n), d_exp.cpu().numpy()


def check_across_args(bands, loading_bands):
    out = []
    for b in (bands, loading_bands):
        b = tuple(float(x) for x in b)
        if len(b) > _lib.ACROSS_MAX_BANDS or not np.isfinite(b).all():
            raise ValueError(f"across report: at most {_lib.ACROSS_MAX_BANDS} finite bands, got {b}")
        out.append(b)
    return out


def across_report_device(volt, loading, groups, nodes=None, rated=None, bands=(0.92, 0.95, 0.98),
                         loading_bands=(0.8, 1.0), vmin=0.95, vmax=1.05, slots=True, lib=None, stream=None) -> AcrossReport:
    """Per node and per line, the statistics across each group's scenarios of voltages and loadings that lie on the
    device: volt, loading contiguous (S, n, T) float64 tensors (study_report's arrays; loading may be None), groups one
    integer per scenario as study_report's (not None).  Nothing but the records is read back.

    nodes           the nodes the voltage records cover (None: all); the others hold empty records
    rated           (n,) ratings or booleans: the loading records cover the lines with rated > 0 (None: all)
    bands           up to 8 voltage thresholds: band_count[b] scenarios at or below bands[b]
    loading_bands   up to 8 loading thresholds: band_count[b] scenarios at or above loading_bands[b]
    vmin / vmax     a voltage outside them is a violation; a loading above 1 is one
    slots           False: no (G, n, T) records, the daily ones and the exposure alone."""
    for name, a in (("volt", volt), ("loading", loading)):
        if a is None and name == "loading":
            continue
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.dim() != 3 or not a.is_contiguous():
            raise ValueError(f"across report: {name} must be a contiguous (scenarios, nodes, slots) float64 tensor")
    if loading is not None and (loading.shape != volt.shape or loading.device != volt.device):
        raise ValueError("across report: volt and loading differ in shape or device")
    S, n, T = volt.shape
    if groups is None:
        raise ValueError("across report: statistics across scenarios need groups (one integer per scenario)")
    _, gid, G = check_study_args(S, (), groups)
    if G < 1:
        raise ValueError("across report: no scenario is in a group")
    bands, loading_bands = check_across_args(bands, loading_bands)
    keep_v = keep_l = None
    if nodes is not None:
        keep_v = np.zeros(n, bool)
        keep_v[np.asarray(nodes)] = True
    if rated is not None:
        keep_l = np.nan_to_num(np.asarray(rated, np.float64), nan=0.0) > 0
        if keep_l.shape != (n,):
            raise ValueError(f"across report: rated must have one entry per node ({n}), got {keep_l.shape}")
    dev = volt.device

    def run(st):
        lb = lib or (_lib.load() if dev.type == "cuda" else None)
        sv, dv, ev = native_across(lb, st, volt, keep_v, gid, G, vmin, vmax, -1, bands, slots)
        sl = dl = el = None
        if loading is not None:
            sl, dl, el = native_across(lb, st, loading, keep_l, gid, G, -np.inf, 1.0, 1, loading_bands, slots)
        return AcrossReport(sv, sl, dv, dl, ev, el, np.bincount(gid[gid >= 0], minlength=G).astype(np.int64), bands,
                            loading_bands)

    return tree_reports.on_device(dev, stream, run)


def native_study_device(lib, dev, stream, tree, tree_host, n_nodes, node_g, groups, n_groups, bands, rating, nodes, vset,
                        vmin, vmax, arrays, across=False) -> StudyReport:
    """revs_net_study on node sums that lie on the device: node_g (S, M, T) float64 device tensor, tree: _lib.Tree (device
    pack / w), tree_host: the dict of feeder_tree, n_nodes: its nodes before padding; groups (S,) int32 in
    -1 .. n_groups - 1.  The one place the library is called from (a host test puts tests/study_ref.py here); the
    records and the S M T node sums are read back.  across=True (with groups): the arrays are written on the device
    whatever `arrays` says, handed to across_report_device before anything is read back -> StudyReport.across, and read
    back themselves only with arrays=True."""
    S, M, T = node_g.shape
    n, B, G = int(n_nodes), len(bands), int(n_groups)
    d_nop, d_rating, d_mask = side_arrays(dev, tree_host, n, rating, nodes)
    out = ([torch.empty(S, n, T, dtype=torch.float64, device=dev) for _ in range(3)] if arrays or across
           else [None] * 3)
    d_sum = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * 2 * T)
    d_pool = d_scratch = d_band = None
    if G:                                   # staging only when pools are asked for
        d_pool = tree_reports.record_buffer(dev, POOLED_DTYPE, G * 2 * T)
        d_scratch = tree_reports.scratch("study report", lib.revs_net_study_scratch(S, T, tree_host["n"]),
                                         f"S={S}, T={T}, tree of {tree_host['n']}", dev, "staging")
    if B:
        d_band = torch.zeros(S, T, B, dtype=torch.int32, device=dev)
    h_group = np.ascontiguousarray(groups, np.int32)
    h_band = np.ascontiguousarray(bands, np.float64)
    check(lib.revs_net_study(S, M, T, C.byref(tree), ptr(node_g), ptr(d_rating), ptr(d_mask), ptr(d_nop), n, float(vset),
                             float(vmin), float(vmax), h_group.ctypes.data if G else None, G,
                             h_band.ctypes.data if B else None, B, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                             ptr(d_sum), ptr(d_pool), ptr(d_band), ptr(d_scratch), stream), "revs_net_study")
    acr = None
    if across:
        acr = across_report_device(out[2], out[1] if rating is not None else None, groups, nodes=nodes, rated=rating,
                                   bands=bands, vmin=vmin, vmax=vmax, lib=lib, stream=stream)
    if not arrays:
        out = [None] * 3
    rec = tree_reports.records(d_sum, SUMMARY_DTYPE, S, 2, T)
    pool = tree_reports.records(d_pool, POOLED_DTYPE, G, 2, T) if G else np.zeros((0, 2, T), POOLED_DTYPE)
    counts = d_band.cpu().numpy() if B else np.zeros((S, T, 0), np.int32)
    flow, loading, volt = (None if o is None else o.cpu().numpy() for o in out)
    return StudyReport(rec[:, 0].copy(), rec[:, 1].copy(), pool[:, 0].copy(), pool[:, 1].copy(), counts,
                       tuple(float(b) for b in bands), np.asarray(groups, np.int64).copy(), flow, loading, volt,
                       node_g.cpu().numpy(), float(vset), float(vmin), float(vmax), acr)


def native_study(parent, edge_r, cons_of, node_p, groups, n_groups, bands, rating, nodes, vset, vmin, vmax, arrays,
                 device, across=False) -> StudyReport:
    """revs_net_study on checked arguments held on the host: node_p (S, M, T) float64, groups (S,) int32 in
    -1 .. n_groups - 1 -- the whole feeder's tree built and the profiles uploaded, then native_study_device."""
    from .engine import _dev_check
    lib, dev = _lib.load(), _dev_check(device)
    with torch.cuda.device(dev):
        th, tree, _keep = tree_on_device(dev, parent, edge_r, cons_of, node_p.shape[1])
        g = torch.from_numpy(node_p).to(dev)
        rep = native_study_device(lib, dev, torch.cuda.current_stream(dev).cuda_stream, tree, th, len(parent), g, groups,
                                  n_groups, bands, rating, nodes, vset, vmin, vmax, arrays, **_across_kw(across))
    rep.node_p = node_p
    return rep


def check_across_groups(across, groups):
    """across=True needs groups with at least one scenario in one: refused before anything is launched."""
    if not across:
        return
    if groups is None:
        raise ValueError("study report: across=True reports across the scenarios of each group: pass groups")
    gid = np.asarray(groups)
    if gid.size and np.issubdtype(gid.dtype, np.integer) and gid.max() < 0:
        raise ValueError("study report: across=True, but no scenario is in a group")


def _across_kw(across):
    """The trailing across=True of native_study / native_study_device, passed only when asked for: a stand-in with
    the signature before it keeps working for every other call."""
    return {"across": True} if across else {}


def check_study_args(S, bands, groups):
    """study_report's checks of S, bands and groups -> (bands, group ids int32 (S,), G)."""
    check_scenarios("study report", S)
    bands = tuple(float(b) for b in bands)
    if len(bands) > _lib.STUDY_MAX_BANDS or not np.isfinite(bands).all():
        raise ValueError(f"study report: at most {_lib.STUDY_MAX_BANDS} finite bands, got {bands}")
    if groups is None:
        return bands, np.full(S, -1, np.int32), 0
    gid = np.asarray(groups)
    if gid.shape != (S,) or not np.issubdtype(gid.dtype, np.integer) or gid.min() < -1:
        raise ValueError(f"study report: groups must be {S} integers >= -1")
    return bands, gid.astype(np.int32), int(gid.max()) + 1


def study_report(parent, edge_r, cons_of, node_p, groups=None, rating=None, nodes=None, bands=(0.92, 0.95, 0.98),
                 vset=1.0, vmin=0.95, vmax=1.05, arrays=False, device="cuda:0", across=False) -> StudyReport:
    """The report of S schedules on one feeder (network.report_for_tree's arguments; node_p is (S, M, T): row
    cons_of[i] of scenario s injected at tree node i).

    groups    None: per-scenario outputs only (no staging is allocated).  Else one integer per scenario: the pool it
              belongs to, 0 .. G-1 with G = max + 1; -1: in none.  pooled_loading / pooled_volt[g] are the box-plot
              numbers over all values of group g's scenarios -- not obtainable from the per-scenario records, since
              quantiles do not compose.
    bands     up to 8 voltage thresholds, any order: band_counts[s, t, b] nodes of `nodes` at or below bands[b].
    nodes     the nodes the voltage summaries, pools and band counts cover (the reference: the community); None: all.
    arrays    True: also flow / loading / volt of every scenario, (S, nodes, T).
    across    True (needs groups): StudyReport.across, the AcrossReport of the voltages and -- with ratings -- the
              loadings: per node and per line the statistics across each group's scenarios, from the arrays on the
              device (across_report_device; `bands` are its voltage bands too)."""
    node_p = np.ascontiguousarray(node_p, np.float64)
    if node_p.ndim != 3:
        raise ValueError(f"study report: node_p must be (scenarios, rows, slots), got {node_p.shape}")
    check_across_groups(across, groups)
    bands, gid, G = check_study_args(node_p.shape[0], bands, groups)
    return native_study(parent, edge_r, cons_of, node_p, gid, G, bands, rating, nodes, vset, vmin, vmax, arrays, device,
                        **_across_kw(across))


def study_report_device(node_g, feeder=None, tree=None, groups=None, rating=None, nodes=None, bands=(0.92, 0.95, 0.98),
                        vset=1.0, vmin=0.95, vmax=1.05, arrays=False, lib=None, stream=None, across=False) -> StudyReport:
    """study_report over node sums that lie on the device: node_g a contiguous (S, M, T) float64 tensor, row
    cons_of[i] of scenario s injected at tree node i (what AdmmEnsemble.node_sums / revs_net_node_sums_many write).
    The feeder comes as feeder=(parent, edge_r, cons_of), study_report's first three arguments -- its tree is built
    and uploaded here -- or as tree=(_lib.Tree, the dict of feeder_tree, nodes before padding) where it already lies
    on node_g's device (an engine's).  Every other argument and check as study_report's; nothing is uploaded but the
    side arrays, and StudyReport.node_p is node_g read back.  lib / stream: the library and the HIP stream of the
    launch (default: the loaded one, torch's current stream)."""
    tree_reports.check_node_sums("study report", node_g, (3,), (feeder, tree), bound=False)
    check_across_groups(across, groups)
    bands, gid, G = check_study_args(node_g.shape[0], bands, groups)
    return tree_reports.run_on_device(
        node_g, feeder, tree,
        lambda *on: native_study_device(*on, gid, G, bands, rating, nodes, vset, vmin, vmax, arrays, **_across_kw(across)),
        lib, stream)
