"""The transformer report: what a schedule does to the service transformers between the primary network and a handful
of homes each -- per transformer and slot the load, the load ratio against the rating, the top-oil and winding hot-spot
temperatures and the ageing acceleration factor (IEEE C57.91 Clause 7: exponential rises, Arrhenius ageing), per
transformer and day the peaks, the energy and the loss of insulation life, per slot the box-plot records over the fleet,
per scenario the fleet's sums and the eight transformers that age most.  Computed on the GPU from node sums that stay on
the device (revs_xf_report: include/revs_admm_ops.h).  It needs no feeder tree.

Limits: active power and one power factor only (rated kW = rated kVA x pf); one thermal model per call; the temperatures
are sampled at the end of each sub-step of a slot, during which the load is constant."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, tree_reports
from ._lib import XF_DAY_DTYPE, XF_FLEET_DTYPE, check, ptr
from .network import SUMMARY_DTYPE, profile_node_sums

STANDARD_KVA = (5.0, 10.0, 15.0, 25.0, 37.5, 50.0, 75.0, 100.0, 167.0)      # single-phase pole-top sizes


@dataclass
class ThermalModel:
    """The usual ONAN 65 K-rise distribution values; every one is a parameter of revs_xf_report (revs_xf_model_t)."""
    dto_r: float = 55.0                 # top-oil rise over ambient at rated load, K
    dhs_r: float = 25.0                 # winding hot-spot rise over top oil at rated load, K
    loss_ratio: float = 5.0             # load loss / no-load loss at rated load
    n: float = 0.8                      # top-oil exponent
    m: float = 0.8                      # winding exponent
    aging_B: float = 15000.0            # Arrhenius constant, K
    theta_ref: float = 110.0            # hot-spot at which the ageing factor is 1, deg C
    normal_life_hours: float = 180000.0
    tau_to: float = 3.0                 # top-oil time constant, h (the decay per sub-step is formed on the host)
    tau_w: float = 0.08                 # winding time constant, h; 0: the winding follows at once

    def struct(self) -> _lib.XfModel:
        vals = {k: float(getattr(self, k)) for k, _ in _lib.XfModel._fields_}
        for k, v in vals.items():
            low = -273.0 if k == "theta_ref" else 0.0
            if not (math.isfinite(v) and v > low):
                raise ValueError(f"transformer report: model {k} must be finite and > {low:g}, got {v}")
        return _lib.XfModel(*vals.values())

    def decays(self, slot_hours, substeps):
        """(decay_to, decay_w) of one sub-step, in double on the host."""
        if not (math.isfinite(self.tau_to) and self.tau_to > 0.0) or not (math.isfinite(self.tau_w) and self.tau_w >= 0.0):
            raise ValueError(f"transformer report: tau_to must be finite and > 0 and tau_w finite and >= 0, got "
                             f"{self.tau_to}, {self.tau_w}")
        h = slot_hours / substeps
        return math.exp(-h / self.tau_to), (math.exp(-h / self.tau_w) if self.tau_w > 0.0 else 0.0)


@dataclass
class TransformerReport:
    """load (kW), ratio, top_oil, hot_spot (deg C), faa: (K, T) float64, or None with arrays=False.  A bad transformer
    (a row that is not finite, a rating that is not finite and > 0) reads NaN in top_oil, hot_spot, faa and in every
    double of its day record.  summary_ratio / summary_hot: (T,) SUMMARY_DTYPE over the transformers, n_violations =
    ratio > over_ratio / hot_spot > hot_limit.  xf_day: (K,) XF_DAY_DTYPE -- peak_ratio, peak_hot and their slots,
    energy_kwh, age_hours, lol_percent, feqa, n_over_slots, n_hot_slots.  fleet: one XF_FLEET_DTYPE record."""
    load: np.ndarray | None
    ratio: np.ndarray | None
    top_oil: np.ndarray | None
    hot_spot: np.ndarray | None
    faa: np.ndarray | None
    summary_ratio: np.ndarray
    summary_hot: np.ndarray
    xf_day: np.ndarray
    fleet: np.ndarray
    rated_kw: np.ndarray
    slot_hours: float
    over_ratio: float = 1.0
    hot_limit: float = 110.0

    @property
    def top_transformers(self):
        """[(transformer, loss of life in % of normal life)] of the up to eight that age most, descending."""
        return [(int(i), float(v)) for i, v in zip(self.fleet["top_index"], self.fleet["top_lol"]) if i >= 0]

    @property
    def overloaded(self):
        """Indices of the transformers above over_ratio in some slot."""
        return np.flatnonzero(self.xf_day["n_over_slots"] > 0)


def build_csr(xf_of, n_rows, K):
    """xf_of: per row of node_g the transformer it belongs to, or -1 -> (xf_ptr int32 (K + 1), xf_rows int32), rows
    ascending within a transformer."""
    xf_of = np.asarray(xf_of)
    if xf_of.shape != (n_rows,) or not np.issubdtype(xf_of.dtype, np.integer):
        raise ValueError(f"transformer report: xf_of must hold one integer per row of node_g ({n_rows}), got "
                         f"{xf_of.shape} {xf_of.dtype}")
    if xf_of.size and (xf_of.min() < -1 or xf_of.max() >= K):
        raise ValueError(f"transformer report: xf_of outside -1..{K - 1}")
    rows = np.flatnonzero(xf_of >= 0)
    rows = rows[np.argsort(xf_of[rows], kind="stable")]
    ptr_ = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(xf_of[rows], minlength=K), out=ptr_[1:])
    return ptr_.astype(np.int32), rows.astype(np.int32)


def native_transformers_device(lib, dev, stream, node_g, xf_ptr, xf_rows, rated_kw, ambient, model=None, slot_hours=None,
                               substeps=1, initial="cyclic", over_ratio=1.0, hot_limit=110.0, arrays=True, out=None) -> list:
    """revs_xf_report on node sums that lie on the device: node_g (S, M, T) float64 device tensor; xf_ptr / xf_rows the
    CSR of build_csr and rated_kw (K,), ambient (T,) as numpy arrays -> S TransformerReports.  The one place the library
    is called from.  out: a contiguous (S, K, T) float64 device tensor that receives the hot-spots and stays there."""
    S, M, T = node_g.shape
    K = len(xf_ptr) - 1
    model = ThermalModel() if model is None else model
    slot_hours = 24.0 / T if slot_hours is None else float(slot_hours)
    over_ratio, hot_limit, substeps = float(over_ratio), float(hot_limit), int(substeps)
    if not (math.isfinite(slot_hours) and slot_hours > 0.0):
        raise ValueError(f"transformer report: slot_hours must be finite and > 0, got {slot_hours}")
    if not 1 <= substeps <= _lib.XF_MAX_SUBSTEPS:
        raise ValueError(f"transformer report: substeps={substeps} outside 1..{_lib.XF_MAX_SUBSTEPS}")
    if math.isnan(over_ratio) or math.isnan(hot_limit):
        raise ValueError("transformer report: over_ratio and hot_limit must be no NaN")
    if isinstance(initial, str):
        if initial != "cyclic":
            raise ValueError(f"transformer report: initial must be 'cyclic' or (to0, w0), got {initial!r}")
        cyclic, to0, w0 = 1, 0.0, 0.0
    else:
        cyclic, (to0, w0) = 0, (float(v) for v in initial)
        if not (math.isfinite(to0) and math.isfinite(w0)):
            raise ValueError(f"transformer report: initial (to0, w0) must be finite, got {(to0, w0)}")
    if not 1 <= K <= 65535:
        raise ValueError(f"transformer report: {K} transformers outside 1..65535")
    rated_kw = np.ascontiguousarray(rated_kw, np.float64)
    ambient = np.ascontiguousarray(ambient, np.float64)
    if rated_kw.shape != (K,):
        raise ValueError(f"transformer report: one rating per transformer ({K}) expected, got {rated_kw.shape}")
    if ambient.shape != (T,):
        raise ValueError(f"transformer report: ambient must be a scalar or one value per slot ({T}), got {ambient.shape}")
    tree_reports.check_out("transformer report", out, (S, K, T), node_g.device)
    mdl = model.struct()
    decay_to, decay_w = model.decays(slot_hours, substeps)
    up = lambda a: torch.tensor(np.asarray(a)).to(dev)           # (a copy: the caller's arrays may be read-only)
    d_ptr, d_rows = up(np.asarray(xf_ptr, np.int32)), up(np.asarray(xf_rows, np.int32))
    d_rated, d_amb = up(rated_kw), up(ambient)
    d_hot = out
    d_load = d_ratio = d_oil = d_faa = None
    if arrays:
        if d_hot is None:
            d_hot = torch.empty(S, K, T, dtype=torch.float64, device=dev)
        d_load, d_ratio, d_oil, d_faa = (torch.empty(S, K, T, dtype=torch.float64, device=dev) for _ in range(4))
    d_sr = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_sh = tree_reports.record_buffer(dev, SUMMARY_DTYPE, S * T)
    d_day = tree_reports.record_buffer(dev, XF_DAY_DTYPE, S * K)
    d_fleet = tree_reports.record_buffer(dev, XF_FLEET_DTYPE, S)
    d_scratch = tree_reports.scratch("transformer report", lib.revs_xf_report_scratch(S, T, K), f"S={S}, T={T}, K={K}", dev)
    check(lib.revs_xf_report(S, M, T, K, len(xf_rows), ptr(node_g), ptr(d_ptr), ptr(d_rows) if len(xf_rows) else None,
                             ptr(d_rated), ptr(d_amb), C.byref(mdl), slot_hours, substeps, decay_to, decay_w, cyclic, to0,
                             w0, over_ratio, hot_limit, ptr(d_load), ptr(d_ratio), ptr(d_oil), ptr(d_hot), ptr(d_faa),
                             ptr(d_sr), ptr(d_sh), ptr(d_day), ptr(d_fleet), ptr(d_scratch), stream), "revs_xf_report")
    sr = tree_reports.records(d_sr, SUMMARY_DTYPE, S, T)
    sh = tree_reports.records(d_sh, SUMMARY_DTYPE, S, T)
    day = tree_reports.records(d_day, XF_DAY_DTYPE, S, K)
    fleet = tree_reports.records(d_fleet, XF_FLEET_DTYPE, S)
    host = [d.cpu().numpy() if arrays else [None] * S for d in (d_load, d_ratio, d_oil, d_hot, d_faa)]
    return [TransformerReport(*(a[s] for a in host), sr[s].copy(), sh[s].copy(), day[s].copy(), fleet[s].copy(), rated_kw,
                              slot_hours, over_ratio, hot_limit) for s in range(S)]


def _ratings(rated_kva, pf, K):
    pf = float(pf)
    if not (math.isfinite(pf) and 0.0 < pf <= 1.0):
        raise ValueError(f"transformer report: pf must lie in (0, 1], got {pf}")
    kva = np.asarray(rated_kva, np.float64)
    if kva.ndim == 0:
        kva = np.full(K, float(kva))
    if kva.shape != (K,):
        raise ValueError(f"transformer report: rated_kva must be a scalar or one value per transformer ({K}), got {kva.shape}")
    return kva * pf


def _ambient(ambient, T):
    a = np.asarray(ambient, np.float64)
    return np.full(T, float(a)) if a.ndim == 0 else a


def transformer_report_device(node_g, xf_of, rated_kva, pf=0.95, ambient=30.0, model=None, slot_hours=None, substeps=1,
                              initial="cyclic", over_ratio=1.0, hot_limit=110.0, arrays=True, out=None, lib=None,
                              stream=None):
    """The transformer report over node sums that lie on the device: node_g a contiguous float64 tensor, (S, M, T) -> a
    list of S TransformerReports, or (M, T) -> one.

    xf_of         per row of node_g, the transformer 0..K-1 it belongs to, or -1 (the row is ignored); K = the length of
                  rated_kva (an array), the CSR is built and validated here on the host
    rated_kva     one rating per transformer; rated kW = rated_kva x pf
    ambient       deg C: a scalar or one value per slot
    model         a ThermalModel; None: its defaults
    slot_hours    hours per slot; None: 24 / T
    substeps      1..16 sub-steps of the recursion per slot
    initial       "cyclic": the day repeats; else (to0, w0), the rises before slot 0
    over_ratio, hot_limit   what n_over_slots / n_hot_slots and the summaries' n_violations count against
    arrays        False: the records only
    out           a contiguous (S, K, T) float64 tensor on node_g's device that receives the hot-spots and stays there,
                  e.g. for revs_net_across (study.native_across) across seeds with hi = hot_limit, sense = +1"""
    single, g3 = tree_reports.check_node_sums("transformer report", node_g)
    K = int(np.asarray(rated_kva).shape[0]) if np.asarray(rated_kva).ndim else int(np.max(xf_of, initial=-1)) + 1
    xf_ptr, xf_rows = build_csr(xf_of, g3.shape[1], max(K, 1))
    rated_kw = _ratings(rated_kva, pf, max(K, 1))
    dev = node_g.device

    def run(st):
        reps = native_transformers_device(lib or _lib.load(), dev, st, g3, xf_ptr, xf_rows, rated_kw,
                                          _ambient(ambient, g3.shape[2]), model, slot_hours, substeps, initial, over_ratio,
                                          hot_limit, arrays, out)
        return reps[0] if single else reps

    return tree_reports.on_device(dev, stream, run)


def report_for_rows(node_p_host, xf_of, rated_kva, device="cuda:0", **kw):
    """The transformer report of node sums held on the host: node_p_host (M, T) or (S, M, T) -> one TransformerReport or
    a list of S (transformer_report_device's arguments)."""
    from .engine import _dev_check
    _lib.load()
    dev = _dev_check(device)
    node_p = np.ascontiguousarray(node_p_host, np.float64)
    with torch.cuda.device(dev):
        return transformer_report_device(torch.from_numpy(node_p).to(dev), xf_of, rated_kva, **kw)


def rows_by_transformer(graph, res=None):
    """-> (the graph's 'T'-labelled nodes in graph order, xf_of): per residence -- in `res` order, by default the 'H'
    nodes in graph order, which is feeder_of's row order -- the index of the transformer that serves it: the nearest
    'T'-labelled node on the way to the 'S' node; -1 where there is none."""
    from .lpsolver import feeder_arrays
    if res is None:
        res = [n for n in graph if graph.nodes[n]["label"] == "H"]
    nonsub = [n for n in graph.nodes if graph.nodes[n]["label"] != "S"]
    parent, _, _ = feeder_arrays(graph, res)
    xf_nodes = [n for n in nonsub if graph.nodes[n]["label"] == "T"]
    index = {n: k for k, n in enumerate(xf_nodes)}
    pos = {n: i for i, n in enumerate(nonsub)}
    owner = np.full(len(nonsub), -2, np.int64)           # per non-substation node, memoised; -2: not known yet

    def find(i):
        path = []
        while i >= 0 and owner[i] == -2 and nonsub[i] not in index:
            path.append(i)
            i = int(parent[i])
        k = -1 if i < 0 else (index[nonsub[i]] if nonsub[i] in index else int(owner[i]))
        owner[path] = k
        return k

    return xf_nodes, np.array([find(pos[h]) for h in res], np.int64)


def size_ratings(peak_kw, pf=0.95, margin=1.0, ladder=STANDARD_KVA):
    """The smallest size of `ladder` (kVA, ascending) at or above margin x peak_kw / pf, per transformer; the largest size
    where the need lies beyond the ladder."""
    ladder = np.asarray(ladder, np.float64)
    if ladder.ndim != 1 or ladder.size == 0 or (np.diff(ladder) <= 0).any() or not (ladder > 0).all():
        raise ValueError("size_ratings: the ladder must be ascending positive sizes")
    need = float(margin) * np.abs(np.asarray(peak_kw, np.float64)) / float(pf)
    return ladder[np.minimum(np.searchsorted(ladder, need, side="left"), ladder.size - 1)]


class TransformerMixin:
    def transformer_report(self, xf_of, rated_kva, profile=None, pf=0.95, ambient=30.0, model=None, slot_hours=None,
                           substeps=1, initial="cyclic", over_ratio=1.0, hot_limit=110.0, arrays=True,
                           out=None) -> TransformerReport:
        """What a home profile does to the service transformers: loading, top-oil and hot-spot temperatures per slot,
        loss of insulation life per day (TransformerReport).

        xf_of         per node row of the engine (0..M-1), the transformer it belongs to, or -1
        rated_kva     one rating per transformer
        profile       as network_report's: None, the schedule's net load LOAD + P_sch; else the residences' net load,
                      (n, T) -- engine.rule_schedule("uncontrolled") or the base load go straight in
        the rest      see transformer_report_device; out is (1, K, T)

        It needs no feeder tree: engines built from a dense R have it too.  With the residences sharded every rank
        returns the whole fleet's report (the all-reduce of the node sums that network_report makes).  The run's state
        is read, never written."""
        node_g = profile_node_sums(self, profile, "transformer_report")
        return transformer_report_device(node_g[None], xf_of, rated_kva, pf, ambient, model, slot_hours, substeps, initial,
                                         over_ratio, hot_limit, arrays, out, lib=self.lib, stream=self.stream)[0]
