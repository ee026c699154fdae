"""ctypes binding of librevs_admm.so (include/revs_admm.h: the boundary; include/revs_admm_ops.h: the operator's
building blocks the Python driver issues one by one).

Loading fails loudly when the library has not been built: nothing in this
package computes on the CPU instead.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (REVS_LIB: a tuning build of the same sources made with `python -m revs_admm_amd.build --out`)
LIB_PATH = os.environ.get("REVS_LIB") or os.path.join(HERE, "librevs_admm.so")

# numpy mirror of revs_home_t (include/revs_admm.h)
HOME_DTYPE = np.dtype([("ev", "<i4"), ("start", "<i4"), ("end", "<i4"), ("nmin", "<i4"),
                       ("nmax", "<i4"), ("rating", "<f4"), ("capacity", "<f4"),
                       ("initial", "<f4")])
assert HOME_DTYPE.itemsize == 32

MODE_BINARY, MODE_RELAXED_PDHG, MODE_RELAXED_EXACT = 0, 1, 2
MODES = {"binary": MODE_BINARY, "relaxed": MODE_RELAXED_PDHG, "pdhg": MODE_RELAXED_PDHG,
         "relaxed_exact": MODE_RELAXED_EXACT}


class PDHG(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("check", C.c_int32), ("tol", C.c_float),
                ("tau_scale", C.c_float), ("sigma_scale", C.c_float), ("full_rows", C.c_int32),
                ("polish", C.c_int32), ("lanes", C.c_int32), ("keys64", C.c_int32)]


class PlanDesc(C.Structure):
    """revs_plan_desc_t"""
    _fields_ = [("n_homes", C.c_int64), ("m", C.c_int32), ("T", C.c_int32),
                ("node_ptr", C.c_void_p), ("R", C.c_void_p), ("Rt", C.c_void_p),
                ("kappa", C.c_double), ("vlo", C.c_double), ("vhi", C.c_double),
                ("kadd", C.c_int32), ("ksplit", C.c_int32),
                ("d_slabs", C.c_void_p), ("v_slabs", C.c_void_p), ("pnq", C.c_void_p),
                ("vfull", C.c_void_p), ("viol", C.c_void_p), ("partial", C.c_void_p),
                ("cand_idx", C.c_void_p), ("cand_cnt", C.c_void_p), ("cand_val", C.c_void_p),
                ("stats", C.c_void_p), ("stats_host", C.c_void_p),
                ("cost", C.c_void_p), ("homes", C.c_void_p), ("load", C.c_void_p),
                ("diff", C.c_void_p), ("dsq", C.c_void_p), ("status", C.c_void_p),
                ("pdhg_dual", C.c_void_p), ("mode", C.c_int32), ("pdhg", PDHG),
                ("node_of", C.c_void_p), ("recompute_pe_new", C.c_int32),
                ("cand_idx1", C.c_void_p), ("cand_cnt1", C.c_void_p), ("cand_val1", C.c_void_p),
                ("stats1", C.c_void_p), ("stats1_host", C.c_void_p),
                ("yhat", C.c_void_p), ("k_full", C.c_void_p), ("info", C.c_void_p),
                ("delta", C.c_double), ("eps", C.c_double), ("max_pivots", C.c_int32)]


class SpecState(C.Structure):
    """revs_spec_state_t"""
    _fields_ = [("p_est", C.c_void_p), ("p_est_new", C.c_void_p), ("p_est_alt", C.c_void_p),
                ("p_sch", C.c_void_p), ("p_sch_alt", C.c_void_p), ("gamma", C.c_void_p),
                ("gamma_alt", C.c_void_p), ("p0", C.c_void_p), ("p_alt", C.c_void_p),
                ("fused_p", C.c_void_p), ("fused_ready", C.c_int32)]


class ChainState(C.Structure):
    """revs_chain_state_t"""
    _fields_ = [("y", C.c_void_p), ("y_trial", C.c_void_p), ("use_y", C.c_int32), ("sup0", C.c_int32),
                ("p_est", C.c_void_p), ("p_est_new", C.c_void_p), ("p_sch", C.c_void_p),
                ("p_sch_alt", C.c_void_p), ("gamma", C.c_void_p), ("gamma_alt", C.c_void_p)]


class ChainFoldState(C.Structure):
    """revs_chain_fold_state_t"""
    _fields_ = [("y", C.c_void_p), ("y_trial", C.c_void_p), ("y_spare", C.c_void_p), ("use_y", C.c_int32),
                ("sup0", C.c_int32), ("p_est", C.c_void_p), ("p_est_new", C.c_void_p), ("p_sch", C.c_void_p),
                ("p_sch_alt", C.c_void_p), ("gamma", C.c_void_p), ("gamma_alt", C.c_void_p),
                ("s_out", C.c_void_p), ("c_out", C.c_void_p), ("resume", C.c_int32), ("pivots", C.c_int32),
                ("redone", C.c_int32), ("p_est_3", C.c_void_p), ("p_sch_3", C.c_void_p), ("gamma_3", C.c_void_p),
                ("pdhg_dual", C.c_void_p), ("pdhg_dual_new", C.c_void_p), ("pdhg_dual_3", C.c_void_p)]


class NewtonOpts(C.Structure):
    """revs_newton_opts_t"""
    _fields_ = [("k_slabs", C.c_void_p), ("nks", C.c_int32), ("alpha_host", C.c_void_p), ("alpha_dev", C.c_void_p),
                ("info_host", C.c_void_p), ("newton_max", C.c_int32), ("ls_max", C.c_int32)]


class NewtonState(C.Structure):
    """revs_newton_state_t"""
    _fields_ = [("y", C.c_void_p), ("y_trial", C.c_void_p), ("use_y", C.c_int32), ("sup", C.c_int32),
                ("p_est", C.c_void_p), ("p_sch", C.c_void_p), ("gamma", C.c_void_p), ("p_est_new", C.c_void_p),
                ("have_first", C.c_int32), ("have_pre", C.c_int32), ("chain_few_in", C.c_int32),
                ("ok", C.c_int32), ("newton", C.c_int32), ("evals", C.c_int32), ("pivots", C.c_int32),
                ("models_small", C.c_int32), ("models_general", C.c_int32), ("last_small", C.c_int32),
                ("few", C.c_int32), ("pre_kept", C.c_int32), ("cur", C.c_int32), ("nsup_sum", C.c_int32),
                ("nsup_max", C.c_int32), ("first_tag", C.c_double), ("pre_tag", C.c_double),
                ("big_needed", C.c_int32), ("_pad", C.c_int32)]


class Tree(C.Structure):
    """revs_tree_t"""
    _fields_ = [("n", C.c_int32), ("pack", C.c_void_p), ("w", C.c_void_p)]


class ChainKvSide(C.Structure):
    """revs_chain_kv_side_t"""
    _fields_ = [("pnq", C.c_void_p), ("y", C.c_void_p), ("vfull", C.c_void_p), ("viol", C.c_void_p),
                ("partial", C.c_void_p), ("cand_idx", C.c_void_p), ("cand_cnt", C.c_void_p), ("cand_val", C.c_void_p),
                ("stats", C.c_void_p), ("seq", C.c_double), ("es", C.c_int32), ("reserved", C.c_int32)]


class ChainKv(C.Structure):
    """revs_chain_kv_t"""
    _fields_ = [("m", C.c_int32), ("T", C.c_int32), ("kadd", C.c_int32), ("has_e2", C.c_int32),
                ("tree", C.POINTER(Tree)), ("vlo", C.c_double), ("vhi", C.c_double), ("kappa", C.c_double),
                ("delta", C.c_double), ("scale", C.c_double), ("eps", C.c_double), ("max_pivots", C.c_int32),
                ("reserved", C.c_int32), ("e1", ChainKvSide), ("e2", ChainKvSide), ("R", C.c_void_p),
                ("k_full", C.c_void_p), ("yhat", C.c_void_p), ("info", C.c_void_p), ("y_trial", C.c_void_p),
                ("lin_out", C.c_void_p), ("clr0", C.c_void_p), ("clr1", C.c_void_p), ("sh_a", C.c_void_p),
                ("sh_b", C.c_void_p), ("prev_cidx", C.c_void_p), ("prev_ccnt", C.c_void_p), ("fwd_src", C.c_void_p),
                ("fwd_dst", C.c_void_p)]


class XfModel(C.Structure):
    """revs_xf_model_t"""
    _fields_ = [("dto_r", C.c_double), ("dhs_r", C.c_double), ("loss_ratio", C.c_double), ("n", C.c_double),
                ("m", C.c_double), ("aging_B", C.c_double), ("theta_ref", C.c_double), ("normal_life_hours", C.c_double)]


class HeadroomAux(C.Structure):
    """revs_headroom_aux_t"""
    _fields_ = [("parent_pos", C.c_void_p), ("wc", C.c_void_p), ("jump", C.c_void_p), ("n_jump", C.c_int32)]


class StreamState(C.Structure):
    """revs_stream_state_t"""
    _fields_ = [("p_est", C.c_void_p * 3), ("p_sch", C.c_void_p * 2), ("gamma", C.c_void_p * 2),
                ("p", C.c_void_p * 3), ("diff_hist", C.c_void_p)]


class StreamSets(C.Structure):
    """revs_stream_sets_t"""
    _fields_ = [("p_est", C.c_void_p * 4), ("p_sch", C.c_void_p * 4), ("gamma", C.c_void_p * 4),
                ("pdhg_dual", C.c_void_p * 4), ("p0", C.c_void_p), ("p0_out", C.c_void_p),
                ("p_est_next", C.c_void_p),
                ("diff_hist", C.c_void_p)]


# revs_host_allreduce_fn
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int32)

TREE_MAX = 16384         # REVS_TREE_MAX
TREE_SWEEP_MAX = 2048    # REVS_TREE_SWEEP_MAX
CHAIN_FOLD_MAX_M = 2048  # REVS_CHAIN_FOLD_MAX_M
STREAM_BLOCK_MAX = 256   # REVS_STREAM_BLOCK_MAX
AGENT_MAX_INNER = 32     # REVS_AGENT_MAX_INNER
STUDY_MAX_S = 4096       # REVS_STUDY_MAX_S
STUDY_MAX_BANDS = 8      # REVS_STUDY_MAX_BANDS
ACROSS_MAX_BANDS = 8     # REVS_ACROSS_MAX_BANDS

# numpy mirror of revs_net_across_t (include/revs_admm_ops.h)
ACROSS_DTYPE = np.dtype([("min", "<f8"), ("q1", "<f8"), ("median", "<f8"), ("q3", "<f8"), ("max", "<f8"), ("mean", "<f8"),
                         ("count", "<i4"), ("n_nan", "<i4"), ("n_violations", "<i4"), ("worst_scenario", "<i4"),
                         ("band_count", "<i4", (ACROSS_MAX_BANDS,))])
assert ACROSS_DTYPE.itemsize == 96

# numpy mirror of revs_bill_summary_t (include/revs_admm_ops.h)
BILL_DTYPE = np.dtype([("min", "<f8"), ("q1", "<f8"), ("median", "<f8"), ("q3", "<f8"), ("max", "<f8"),
                       ("whisker_lo", "<f8"), ("whisker_hi", "<f8"), ("total", "<f8"), ("reserved0", "<f8"),
                       ("count", "<i4"), ("n_nan", "<i4"), ("n_fliers", "<i4"), ("n_above", "<i4"),
                       ("worst_index", "<i4"), ("worst_scenario", "<i4")])
assert BILL_DTYPE.itemsize == 96

# numpy mirrors of revs_conv_res_t and revs_conv_run_t (include/revs_admm_ops.h)
CONV_RES_DTYPE = np.dtype([("max", "<f4"), ("last", "<f4"), ("settle", "<i4"), ("n_above", "<i4"),
                           ("worst_iteration", "<i4"), ("reserved", "<i4")])
assert CONV_RES_DTYPE.itemsize == 24
CONV_RUN_DTYPE = np.dtype([("converged_at", "<i4"), ("last_above", "<i4"), ("n_unsettled", "<i4"), ("n_never", "<i4")])
assert CONV_RUN_DTYPE.itemsize == 16

# numpy mirror of revs_profile_day_t (include/revs_admm_ops.h)
PROFILE_DAY_DTYPE = np.dtype([("peak", "<f8"), ("valley", "<f8"), ("energy", "<f8"), ("load_factor", "<f8"),
                              ("sum_peaks", "<f8"), ("diversity", "<f8"), ("peak_slot", "<i4"), ("valley_slot", "<i4"),
                              ("slots", "<i4"), ("reserved", "<i4")])
assert PROFILE_DAY_DTYPE.itemsize == 64
PROFILE_MAX_CLASSES = 4  # REVS_PROFILE_MAX_CLASSES

# numpy mirrors of revs_charge_row_t, revs_charge_slot_t and revs_charge_day_t (include/revs_admm_ops.h)
CHARGE_ROW_DTYPE = np.dtype([("energy", "<f8"), ("cost", "<f8"), ("soc_end", "<f4"), ("reserved0", "<f4"),
                             ("n_on", "<i4"), ("n_full", "<i4"), ("first_on", "<i4"), ("last_on", "<i4"),
                             ("sessions", "<i4"), ("wait", "<i4"), ("n_outside", "<i4"), ("flags", "<i4"),
                             ("reserved", "<i4", (2,))])
assert CHARGE_ROW_DTYPE.itemsize == 64
CHARGE_SLOT_DTYPE = np.dtype([("n_ev", "<i4"), ("n_plugged", "<i4"), ("n_on", "<i4"), ("n_full", "<i4"),
                              ("n_starts", "<i4"), ("reserved", "<i4"), ("power", "<f8")])
assert CHARGE_SLOT_DTYPE.itemsize == 32
CHARGE_DAY_DTYPE = np.dtype([("peak_power", "<f8"), ("energy", "<f8"), ("coincidence", "<f8"), ("cost", "<f8"),
                             ("peak_on", "<i4"), ("peak_on_slot", "<i4"), ("peak_power_slot", "<i4"), ("n_ev", "<i4"),
                             ("n_under", "<i4"), ("n_never", "<i4"), ("n_interrupted", "<i4"), ("n_outside", "<i4")])
assert CHARGE_DAY_DTYPE.itemsize == 64
CHARGE_EV, CHARGE_UNDER, CHARGE_NONFINITE = 1, 2, 4      # bits of revs_charge_row_t.flags

# numpy mirrors of revs_flex_row_t, revs_flex_slot_t and revs_flex_day_t (include/revs_admm_ops.h)
FLEX_ROW_DTYPE = np.dtype([("up_energy", "<f8"), ("down_energy", "<f8"), ("laxity", "<f8"), ("energy", "<f8"),
                           ("ready", "<i4"), ("slack", "<i4"), ("n_up", "<i4"), ("n_down", "<i4"), ("flags", "<i4"),
                           ("reserved", "<i4", (3,))])
assert FLEX_ROW_DTYPE.itemsize == 64
FLEX_SLOT_DTYPE = np.dtype([("n_plugged", "<i4"), ("n_up", "<i4"), ("n_down", "<i4"), ("reserved", "<i4"),
                            ("up", "<f8"), ("down", "<f8")])
assert FLEX_SLOT_DTYPE.itemsize == 32
FLEX_DAY_DTYPE = np.dtype([("up_energy", "<f8"), ("down_energy", "<f8"), ("peak_up", "<f8"), ("peak_down", "<f8"),
                           ("peak_up_slot", "<i4"), ("peak_down_slot", "<i4"), ("n_ev", "<i4"), ("n_never_ready", "<i4"),
                           ("n_unservable", "<i4"), ("n_late", "<i4"), ("n_rigid", "<i4"), ("reserved", "<i4")])
assert FLEX_DAY_DTYPE.itemsize == 64
# bits of revs_flex_row_t.flags
FLEX_EV, FLEX_NEVER_READY, FLEX_NONFINITE, FLEX_UNSERVABLE, FLEX_LATE = 1, 2, 4, 8, 16

# numpy mirror of revs_headroom_day_t (include/revs_admm_ops.h)
HEADROOM_DAY_DTYPE = np.dtype([("min", "<f8"), ("slot", "<i4"), ("n_short", "<i4")])
assert HEADROOM_DAY_DTYPE.itemsize == 16
HEADROOM_MAX_JUMP = 13   # REVS_HEADROOM_MAX_JUMP

# numpy mirrors of revs_loss_slot_t, revs_loss_line_day_t, revs_loss_day_t (include/revs_admm_ops.h)
LOSS_SLOT_DTYPE = np.dtype([("total", "<f8"), ("delivered", "<f8"), ("class_total", "<f8", (4,)), ("mlf_max", "<f8"),
                            ("mlf_max_index", "<i4"), ("n_bad", "<i4")])
assert LOSS_SLOT_DTYPE.itemsize == 64
LOSS_LINE_DAY_DTYPE = np.dtype([("energy", "<f8"), ("peak", "<f8"), ("peak_slot", "<i4"), ("reserved", "<i4")])
assert LOSS_LINE_DAY_DTYPE.itemsize == 24
LOSS_DAY_DTYPE = np.dtype([("energy", "<f8"), ("delivered", "<f8"), ("class_energy", "<f8", (4,)), ("cost", "<f8"),
                           ("peak", "<f8"), ("top_energy", "<f8", (8,)), ("top_index", "<i4", (8,)), ("peak_slot", "<i4"),
                           ("n_bad_slots", "<i4"), ("reserved", "<i4", (6,))])
assert LOSS_DAY_DTYPE.itemsize == 192
LOSS_MAX_CLASSES = 4

# numpy mirrors of revs_attr_slot_t and revs_attr_day_t (include/revs_admm_ops.h)
ATTR_SLOT_DTYPE = np.dtype([("drop_watch", "<f8"), ("excess", "<f8"), ("total", "<f8"), ("ev_total", "<f8"),
                            ("class_total", "<f8", (4,)), ("top_value", "<f8", (8,)), ("top_index", "<i4", (8,)),
                            ("watch", "<i4"), ("n_reach", "<i4"), ("n_big", "<i4"), ("n_can", "<i4"), ("n_bad", "<i4"),
                            ("reserved", "<i4", (3,))])
assert ATTR_SLOT_DTYPE.itemsize == 192
ATTR_DAY_DTYPE = np.dtype([("sum", "<f8"), ("ev_sum", "<f8"), ("peak", "<f8"), ("peak_slot", "<i4"), ("n_big", "<i4")])
assert ATTR_DAY_DTYPE.itemsize == 32
ATTR_MAX_CLASSES = 4

# numpy mirrors of revs_risk_slot_t and revs_risk_day_t (include/revs_admm_ops.h)
RISK_SLOT_DTYPE = np.dtype([("expected", "<f8"), ("z_min", "<f8"), ("sd_at", "<f8"), ("drop_at", "<f8"), ("sd_max", "<f8"),
                            ("n_risky", "<i4"), ("n_det", "<i4"), ("z_min_index", "<i4"), ("n_bad", "<i4"),
                            ("reserved", "<i4", (2,))])
assert RISK_SLOT_DTYPE.itemsize == 64
RISK_DAY_DTYPE = np.dtype([("prob_max", "<f8"), ("z_min", "<f8"), ("expected_slots", "<f8"), ("prob_max_slot", "<i4"),
                           ("n_risky", "<i4")])
assert RISK_DAY_DTYPE.itemsize == 32
RISK_MAX_COMMON = 2      # REVS_RISK_MAX_COMMON

# numpy mirrors of revs_price_slot_t, revs_price_node_day_t and revs_price_day_t (include/revs_admm_ops.h); the lines' day
# records are LOSS_LINE_DAY_DTYPE
PRICE_SLOT_DTYPE = np.dtype([("delivered", "<f8"), ("energy_pay", "<f8"), ("loss_pay", "<f8"), ("cong_pay", "<f8"),
                             ("rent_total", "<f8"), ("price_max", "<f8"), ("price_min", "<f8"), ("cong_max", "<f8"),
                             ("price_max_index", "<i4"), ("price_min_index", "<i4"), ("cong_max_index", "<i4"),
                             ("n_priced", "<i4"), ("n_rows", "<i4"), ("n_bad", "<i4"), ("reserved", "<i4", (2,))])
assert PRICE_SLOT_DTYPE.itemsize == 96
PRICE_NODE_DAY_DTYPE = np.dtype([("paid", "<f8"), ("cong_paid", "<f8"), ("peak_price", "<f8"), ("peak_slot", "<i4"),
                                 ("reserved", "<i4")])
assert PRICE_NODE_DAY_DTYPE.itemsize == 32
PRICE_DAY_DTYPE = np.dtype([("energy_pay", "<f8"), ("loss_pay", "<f8"), ("cong_pay", "<f8"), ("rent_total", "<f8"),
                            ("peak_price", "<f8"), ("top_rent", "<f8", (8,)), ("top_index", "<i4", (8,)),
                            ("peak_slot", "<i4"), ("peak_index", "<i4"), ("n_bad_slots", "<i4"), ("n_cong_slots", "<i4"),
                            ("reserved", "<i4", (2,))])
assert PRICE_DAY_DTYPE.itemsize == 160

# numpy mirrors of revs_pf_slot_t, revs_pf_node_day_t and revs_pf_day_t (include/revs_admm_ops.h)
PF_SLOT_DTYPE = np.dtype([("loss_total", "<f8"), ("qloss_total", "<f8"), ("delivered", "<f8"), ("supplied", "<f8"),
                          ("volt_min", "<f8"), ("err_max", "<f8"), ("volt_min_index", "<i4"), ("err_index", "<i4"),
                          ("n_below", "<i4"), ("n_below_lin", "<i4"), ("n_missed", "<i4"), ("iters", "<i4"),
                          ("status", "<i4"), ("reserved", "<i4")])
assert PF_SLOT_DTYPE.itemsize == 80
PF_NODE_DAY_DTYPE = np.dtype([("volt_min", "<f8"), ("slot", "<i4"), ("slots_below", "<i4"), ("slots_missed", "<i4"),
                              ("reserved", "<i4")])
assert PF_NODE_DAY_DTYPE.itemsize == 24
PF_DAY_DTYPE = np.dtype([("energy_lost", "<f8"), ("energy_delivered", "<f8"), ("cost", "<f8"), ("volt_min", "<f8"),
                         ("volt_min_slot", "<i4"), ("volt_min_index", "<i4"), ("n_below", "<i4"), ("n_below_lin", "<i4"),
                         ("n_missed", "<i4"), ("iters_max", "<i4"), ("n_bad_slots", "<i4"), ("reserved", "<i4")])
assert PF_DAY_DTYPE.itemsize == 64
PF_MAX_ITER = 64         # REVS_PF_MAX_ITER

# numpy mirrors of revs_xf_day_t and revs_xf_fleet_t (include/revs_admm_ops.h)
XF_DAY_DTYPE = np.dtype([("peak_ratio", "<f8"), ("peak_hot", "<f8"), ("energy_kwh", "<f8"), ("age_hours", "<f8"),
                         ("lol_percent", "<f8"), ("feqa", "<f8"), ("peak_ratio_slot", "<i4"), ("peak_hot_slot", "<i4"),
                         ("n_over_slots", "<i4"), ("n_hot_slots", "<i4")])
assert XF_DAY_DTYPE.itemsize == 64
XF_FLEET_DTYPE = np.dtype([("lol_sum", "<f8"), ("lol_max", "<f8"), ("energy_kwh", "<f8"), ("feqa_mean", "<f8"),
                           ("top_lol", "<f8", (8,)), ("top_index", "<i4", (8,)), ("n_xf", "<i4"), ("n_nan", "<i4"),
                           ("n_overloaded", "<i4"), ("n_hot", "<i4"), ("n_aging", "<i4"), ("reserved", "<i4", (3,))])
assert XF_FLEET_DTYPE.itemsize == 160
XF_MAX_SUBSTEPS = 16


class RevsError(RuntimeError):
    pass


_p = C.c_void_p
_i32, _i64, _f32, _f64 = C.c_int32, C.c_int64, C.c_float, C.c_double

# name -> (restype, argtypes); every symbol include/revs_admm.h and include/revs_admm_ops.h declare
SIGNATURES = {
    "revs_version": (C.c_char_p, []),
    "revs_last_error": (C.c_char_p, []),
    "revs_host_device_ptr": (C.c_int, [_p, C.POINTER(C.c_void_p)]),
    "revs_plan_create": (C.c_void_p, [C.POINTER(PlanDesc)]),
    "revs_plan_destroy": (None, [_p]),
    "revs_plan_chain_step": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                      _p, _p, _p, _p]),
    "revs_plan_chain_run": (C.c_int, [_p, _i32, C.POINTER(ChainState), _i32, _p, _p]),
    "revs_plan_chain_fold_run": (C.c_int, [_p, _i32, C.POINTER(ChainFoldState), _p, _p]),
    "revs_plan_spec_run": (C.c_int, [_p, _i32, _p, C.POINTER(SpecState), _f64, _f64, _p, _p, _p, _p]),
    "revs_plan_spec_step": (C.c_int, [_p, _i32, _p, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p,
                                      _p, _p, C.POINTER(C.c_double), _p, _p, _p]),
    "revs_op_dual_rows": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _f64, _f64, _p, _p, _p, _p, _p]),
    "revs_pdhg_defaults": (None, [C.POINTER(PDHG)]),
    "revs_residual_num_chunks": (_i32, [_i64]),
    "revs_agent_step": (C.c_int, [_i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                  _f32, _i32, C.POINTER(PDHG), _p]),
    "revs_agent_step_out": (C.c_int, [_i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                      _p, _p, _f32, _i32, C.POINTER(PDHG), _p]),
    "revs_agent_step_select": (C.c_int, [_i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                         _p, _p, _p, _f32, _i32, C.POINTER(PDHG), _i32, _p, _p,
                                         _f64, _f64, _i32, _p, _p, _p, _p, _p, _p, _f64, _p, _p, _p,
                                         _i32, _p]),
    "revs_agent_max_inner": (C.c_int32, [C.c_int32, C.c_int32]),
    "revs_agent_step_multi": (C.c_int, [_i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p,
                                        _p, _p, _f32, _i32, C.POINTER(PDHG), _p, _p, _i64, _p, _i32, _p]),
    "revs_op_dual_product_rows": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _f64, _f64, _i32, _p, _p, _p,
                                            _p, _p, _p, _p]),
    "revs_residual_finalize": (C.c_int, [_p, _p, _i64, _i32, _f32, _f32, _p, _p, _p]),
    "revs_residence_solve": (C.c_int, [_i64, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "revs_dual_bound": (C.c_int, [_i64, _i32, _p, _p, _p, _i32, _p, _p, _p, _f64, _f64, _f64, _i32, _p, _p, _p, _p]),
    "revs_dual_bound_scratch": (_i64, [_i64, _i32]),
    "revs_dual_bound_many": (C.c_int, [_i64, _i32, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _f64, _f64, _i32, _p, _p, _p]),
    "revs_dual_bound_many_scratch": (_i64, [_i64, _i32, _i32]),
    "revs_gemm_tn_f64": (C.c_int, [_i32, _i32, _i32, _p, _i32, _p, _i32, _p, _i32, _i32, _p]),
    "revs_gemm_tn_f32": (C.c_int, [_i32, _i32, _i32, _p, _i32, _p, _i32, _p, _i32, _i32, _p]),
    "revs_gemm_tn_f64_split": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _i32, _p]),
    "revs_gemm_tn_f64_x2": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _i32, _p]),
    "revs_gemm_tn_f64_cat": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _i32, _p]),
    "revs_voltage_f32": (C.c_int, [_i32, _i32, _p, _p, _p, _p]),
    "revs_aggregate_f64": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p]),
    "revs_aggregate_f32": (C.c_int, [_i32, _i32, _p, _p, _p, _p]),
    "revs_op_g0": (C.c_int, [_i64, _i32, _p, _p, _p, _f32, _p, _p]),
    "revs_op_init_home": (C.c_int, [_i64, _i32, _p, _p, _p]),
    "revs_op_init_node": (C.c_int, [_i32, _i32, _p, _p, _p, _f64, _f64, _p, _p, _p, _p]),
    "revs_op_home_pass": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _p, _f64, _f64, _p, _p, _p,
                                    _p]),
    "revs_op_home_pass_fused": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _f64, _p, _i32, _p,
                                          _p, _p, _p, _f64, _f64, _p, _p, _p, _p, _p]),
    "revs_op_node_w": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p]),
    "revs_op_row_scale": (C.c_int, [_i32, _i32, _p, _p, _p, _p]),
    "revs_op_node_scale": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _f64, _p, _p, _p]),
    "revs_op_node_update": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _f64, _f64, _f64,
                                      _f64, _p, _p, _p, _p, _p, _p]),
    "revs_op_node_prep": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _i32, _p, _p, _p, _p]),
    "revs_op_nodefast_feas": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _f64, _f64, _p, _p, _p]),
    "revs_op_nodefast_scale": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _f64, _p, _p, _p]),
    "revs_op_nodefast_update": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _f64, _f64, _f64, _p, _p,
                                          _p, _p, _p]),
    "revs_op_nodefast_dualres": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _f64, _p, _p]),
    "revs_op_nodefast_finish": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_op_node_apply": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _i32, _p, _p, _p]),
    "revs_op_export": (C.c_int, [_i64, _i32, _p, _p, _p]),
    "revs_op_dual_eval": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _i32, _p, _f64, _p, _p, _p]),
    "revs_op_dual_eval_rows": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _f64, _p, _p, _p]),
    "revs_op_dual_blocks": (_i32, [_i32]),
    "revs_op_dual_select": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _f64, _f64, _i32, _p, _p, _p,
                                      _p, _p, _p, _p, _f64, _p]),
    "revs_op_dual_model": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _f64, _i32, _i32, _p,
                                     _p, _p, _p, _p]),
    "revs_op_dual_evaluate": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i32, _f64,
                                        _f64, _f64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                        _p, _p, _f64, _p, _p]),
    "revs_op_dual_model_small": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _f64, _i32, _p, _p,
                                           _p, _p]),
    "revs_op_dual_step": (C.c_int, [_i32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_op_dual_select_big": (C.c_int, [_i32, _i32, _p, _p, _p, _f64, _f64, _i32, _p, _p, _p, _p]),
    "revs_op_dual_model_big": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p, _f64, _f64, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "revs_op_dual_step_big": (C.c_int, [_i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p]),
    "revs_op_dual_select_model_step": (C.c_int, [_i32, _i32, _p, _i32, _p, _f64, _f64, _i32, _p, _p, _p,
                                                _p, _p, _p, _f64, _p, _p, _f64, _f64, _i32, _p, _p, _p,
                                                _f64, _f64, _p, _p, _p]),
    "revs_op_dual_rows_tree": (C.c_int, [_i32, _i32, C.POINTER(Tree), _p, _p, _f64, _f64, _i32, _p, _p, _p, _p,
                                         _p, _p, _p, _p, _f64, _i32, _p]),
    "revs_op_dual_evaluate_tree": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p, C.POINTER(Tree), _p, _i32,
                                             _f64, _f64, _f64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                             _p, _f64, _p]),
    "revs_op_dual_tree_select_model_step": (C.c_int, [_i32, _i32, C.POINTER(Tree), _p, _p, _f64, _f64, _i32, _p,
                                                      _p, _p, _p, _p, _p, _p, _f64, _p, _f64, _f64, _i32, _p, _p,
                                                      _p, _f64, _f64, _p, _p, _p]),
    "revs_op_chain_kv": (C.c_int, [C.POINTER(ChainKv), _p]),
    "revs_newton_chain_accept": (C.c_int, [_i32, _p, _p, _f64, _f64, _i32, _i32, _i32, _p, _p]),
    "revs_tree_voltage": (C.c_int, [_i32, _i32, C.POINTER(Tree), _p, _f64, _f64, _p, _p, _p]),
    "revs_comm_unique_id": (C.c_int, [_p]),
    "revs_comm_create": (C.c_void_p, [_p, _i32, _i32]),
    "revs_comm_create_hook": (C.c_void_p, [_p, _p, _i32, _i32]),
    "revs_comm_destroy": (None, [_p]),
    "revs_comm_allreduce_f64": (C.c_int, [_p, _p, _i64, _i32, _p]),
    "revs_plan_set_tree": (C.c_int, [_p, C.POINTER(Tree)]),
    "revs_plan_set_comm": (C.c_int, [_p, _p]),
    "revs_plan_set_stream_block": (C.c_int, [_p, C.c_int32, C.c_int32]),
    "revs_plan_set_stream_inner": (C.c_int, [_p, C.c_int32]),
    "revs_plan_set_fold_redo": (C.c_int, [_p, C.c_int32]),
    "revs_plan_set_kadd_cold": (C.c_int, [_p, C.c_int32, C.c_int32]),
    "revs_plan_prepare": (C.c_int, [_p]),
    "revs_status_or": (C.c_int, [C.c_int64, _p, _p, _p]),
    "revs_plan_set_newton": (C.c_int, [_p, C.POINTER(NewtonOpts)]),
    "revs_plan_newton_solve": (C.c_int, [_p, C.POINTER(NewtonState), _p]),
    "revs_plan_set_pdhg_dual": (C.c_int, [_p, _p]),
    "revs_plan_stream_run_blocks": (C.c_int, [_p, _i32, C.POINTER(StreamSets), _f64, _f64, _p, _p, _p, _p]),
    "revs_plan_stream_timing": (C.c_int, [_p, C.c_int32]),
    "revs_plan_stream_elapsed_ms": (C.c_int, [_p, _p]),
    "revs_plan_stream_launches": (_i64, [_p]),
    "revs_plan_collective_ms": (C.c_int, [_p, _p, _p, _p]),
    "revs_plan_stream_run": (C.c_int, [_p, _i32, C.POINTER(StreamState), _f64, _f64, _p, _p, _p]),
    "revs_plan_status_flags": (_i32, [_p, _i32]),
    "revs_net_node_sums": (C.c_int, [_i32, _i32, _p, _p, _p, _p, _p]),
    "revs_net_node_sums_many": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _p, _p]),
    "revs_net_report": (C.c_int, [_i32, _i32, C.POINTER(Tree), _p, _p, _p, _p, _i32, _f64, _f64, _f64, _p, _p, _p, _p, _p]),
    "revs_net_study_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_study": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), _p, _p, _p, _p, _i32, _f64, _f64, _f64, _p, _i32, _p,
                                 _i32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_across_scratch": (_i64, [_i32, _i32]),
    "revs_net_across": (C.c_int, [_i32, _i32, _i32, _p, _p, _p, _i32, _f64, _f64, _i32, _p, _i32, _p, _p, _p, _p, _p]),
    "revs_bill_rows": (C.c_int, [_i32, _i64, _i32, _p, _i32, _i64, _i64, _p, _p, _p]),
    "revs_bill_study_scratch": (_i64, [_i32, _i64]),
    "revs_bill_study": (C.c_int, [_i32, _i64, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _p, _p]),
    "revs_conv_report_scratch": (_i64, [_i32, _i64, _i32, _i32]),
    "revs_conv_report": (C.c_int, [_i32, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _f64, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "revs_rule_schedule": (C.c_int, [_i64, _i32, _p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p]),
    "revs_load_profile_chunk": (_i32, []),
    "revs_load_profile_scratch": (_i64, [_i32, _i64, _i32, _i32, _i32]),
    "revs_load_profile": (C.c_int, [_i32, _i64, _i32, _p, _i64, _i64, _p, _i32, _p, _p, _i32, _f64, _p, _p, _p, _p, _p, _p,
                                    _p]),
    "revs_charge_report_chunk": (_i32, []),
    "revs_charge_report_scratch": (_i64, [_i32, _i64, _i32]),
    "revs_charge_report": (C.c_int, [_i32, _i64, _i32, _p, _i64, _i64, _p, _p, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_op_dual_step_pending": (C.c_int, [_i32, _p, _p, _p, _p, _p, _f64, _f64, _p, _i32, _p, _p, _p]),
    "revs_net_headroom_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_headroom": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), C.POINTER(HeadroomAux), _p, _p, _p, _p, _p, _i32, _f64,
                                    _f64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_losses_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_losses": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), _p, _p, _p, _p, _i32, _p, _i32, _f64, _f64, _f64, _p,
                                  _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_attribution_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_attribution": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), C.POINTER(HeadroomAux), _p, _p, _p, _p, _p, _i32,
                                       _p, _i32, _i32, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_risk_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_risk": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), C.POINTER(HeadroomAux), _p, _p, _p, _i32, _p, _p, _p, _p,
                                _i32, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_prices_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_prices": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), _p, _p, _p, _p, _p, _p, _p, _i32, _f64, _i32, _f64, _f64,
                                  _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_net_powerflow_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_net_powerflow": (C.c_int, [_i32, _i32, _i32, C.POINTER(Tree), _p, _p, _f64, _p, _p, _i32, _f64, _f64, _f64, _i32,
                                     _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_xf_report_scratch": (_i64, [_i32, _i32, _i32]),
    "revs_xf_report": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, C.POINTER(XfModel), _f64, _i32, _f64,
                                 _f64, _i32, _f64, _f64, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "revs_flex_report_chunk": (_i32, []),
    "revs_flex_report_scratch": (_i64, [_i32, _i64, _i32]),
    "revs_flex_report": (C.c_int, [_i32, _i64, _i32, _p, _i64, _i64, _p, _i32, _f64, _f64, _p, _i32, _p, _p, _p, _p, _p, _p,
                                   _p, _p, _p, _p]),
}
DUAL_AMAX = 128          # REVS_DUAL_AMAX
DUAL_FEW = 48            # REVS_DUAL_FEW (16 / 32: the same times on the 121144 feeder; 80 / 128: 11.2 ms against 9.5, r05)
DUAL_AMAX_BIG = 512      # REVS_DUAL_AMAX_BIG
ENS_MAX_COLS = 1024      # REVS_ENS_MAX_COLS: columns (scenarios x slots) of one dual Newton launch
MAX_T = 192              # REVS_MAX_T: slots of a residence sweep, columns of a dense product
RULE_ASAP, RULE_ALAP, RULE_EVEN = 0, 1, 2    # REVS_RULE_*: revs_rule_schedule's policies
FILL_TARGET, FILL_FULL = 0, 1                # REVS_FILL_*

_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raise (never fall back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RevsError(
            f"{LIB_PATH} is missing: build it with `python -m revs_admm_amd.build` "
            "(hipcc, gfx950).  revs_admm_amd has no CPU fallback.")
    # PyTorch-ROCm carries its own libamdhip64; load it FIRST so that this library's
    # NEEDED libamdhip64.so.7 resolves to the runtime torch's tensors and streams live
    # in.  (Loaded the other way round the process ends up with two HIP runtimes and
    # the second one finds "no ROCm-capable device".)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().revs_last_error().decode()
        raise RevsError(f"{what or 'librevs_admm'} failed ({rc}): {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
