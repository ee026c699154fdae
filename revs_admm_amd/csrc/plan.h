// Private to the plan runtime (runtime.cpp, plan_newton.cpp, plan_fold.cpp, plan_stream.cpp, comm.cpp): the plan and
// communicator structs, the functions these files share and the steps their native loops have in common.
#pragma once
#include "common.h"
#include "internal.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <vector>

// A communicator (revs_comm_create / _create_hook, comm.cpp); the plan's loops read rank and nranks.
struct revs_comm {
    void *nccl;                             // RCCL communicator, or NULL: the caller's own transport
    int rank, nranks;
    revs_host_allreduce_fn fn = nullptr;    // host-staged all-reduce supplied by the caller
    void *ctx = nullptr;
    double *stage = nullptr;                // pinned staging buffer of the hook form
    size_t stage_count = 0;
};

// ---- steady-state ADMM iteration as one host call (see revs_admm.h) -------------------
struct revs_plan {
    revs_plan_desc_t d;
    hipEvent_t ev;
    double seq;
    uint32_t *counters;     // device, one per 32-row tile: K-split workgroups of R p done
    double t_launch = 0.0, t_wait = 0.0;   // host time in launches / waiting (REVS_PLAN_TRACE)
    // streaming steady state (revs_plan_stream_run)
    revs::StreamCtl *ctl = nullptr;        // device
    double *rec_host = nullptr;            // pinned: double[kRecRing][4] = {rmax, failed, seq, max diff of the iteration before}
    double *rec_dev = nullptr;             // its device-side address
    unsigned int *flags_host = nullptr;    // pinned: OR of the residences' status bits
    unsigned int *flags_dev = nullptr;
    unsigned int stream_seq = 0;           // sequence number of the last streaming launch
    revs::TreeArgs tree{};                 // tree.n == 0: no tree form
    revs_comm *comm = nullptr;
    // verdicts by blocks (revs_plan_set_stream_block)
    int32_t block = 0;                     // iterations judged together; <= 1: every launch judges itself
    int32_t overlap = 0;                   // all-reduce + verdicts of a block on `side`, beside the next block's sweeps
    int32_t inner = 1;                     // ADMM iterations per sweep launch (revs_plan_set_stream_inner)
    int32_t fold_redo = 2;                 // Newton steps beyond the first inside the folded chain (revs_plan_set_fold_redo)
    int32_t kadd_cold = 0, kadd_cold_at = 0;   // revs_plan_set_kadd_cold: rows admitted per Newton iteration while many are violated
    int32_t *wg_order = nullptr;           // the sweep's workgroups, heaviest first (plan_wg_order), device; built on first use
    bool wg_order_tried = false;           // plan_wg_order has run (wg_order: its result, NULL included)
    double *ring = nullptr;                // device: node sums (+ diff tails) of two blocks, double[2][block][stride]
    size_t ring_cap = 0;                   // ... doubles allocated
    bool ring_dirty = true;                // the ring is not known to be all zero (fresh, or a call failed)
    unsigned long long *grp_bits = nullptr;                // device: per-slice maxima, zero between launches
    double *grp_dmax = nullptr;            // device: per-slice max diff
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> events;        // pool: sweeps-done / verdicts-done per block, end of call
    // optional timing of the bursts on their own stream (revs_plan_stream_timing)
    hipEvent_t tev[2] = {nullptr, nullptr};
    hipEvent_t cev[4] = {nullptr, nullptr, nullptr, nullptr};   // around a block's all-reduce / around that block's sweeps
    bool cev_valid = false;
    int32_t cev_nb = 0;                    // iterations of the timed block
    // folded chain (revs_plan_chain_fold_run): sums of the trial's evaluation E2 / of the next
    // iteration's evaluation E1 by iteration parity, the E2 side's row scratch, the odd parity's
    // candidate sets and stats blocks ([0]: the evaluation's, [1]: the trial's)
    double *fold_e2[2] = {nullptr, nullptr}, *fold_e1[2] = {nullptr, nullptr};
    double *fold_v[3] = {nullptr, nullptr, nullptr};
    int32_t *fold_info[2] = {nullptr, nullptr};        // the models' pivot counts, by iteration parity
    double *fold_sh[2] = {nullptr, nullptr};           // the trial's shifts R^T y / kappa, list order / row order
    int64_t *fold_ci[2] = {nullptr, nullptr};
    int32_t *fold_cc[2] = {nullptr, nullptr};
    double *fold_cv[2] = {nullptr, nullptr};
    double *fold_st_host[2] = {nullptr, nullptr}, *fold_st_dev[2] = {nullptr, nullptr};
    revs_newton_opts_t newton{};           // revs_plan_set_newton
    double *fold_st_local[2] = {nullptr, nullptr};     // device: stats of the next-iteration half, by the parity of the set they belong to
    bool fold_st_local_valid = false;      // ... hold the stats of the evaluation the next verdict belongs to
    int32_t fold_par = 0;                  // parity of the iteration a resumed call starts with
    bool fold_ready = false;               // ... whose rows / model / step the last call has already run
    int32_t timing = 0;                    // 0 off, 1 armed (next burst records tev[0]), 2 open
    int64_t timed_launches = 0;            // residence-sweep launches between the two events
};

// Shared between the plan's files; hidden: not part of the library's exported symbols.
#define REVS_PLAN_PRIVATE __attribute__((visibility("hidden")))
REVS_PLAN_PRIVATE const int32_t *plan_wg_order(revs_plan_t *plan);                        // runtime.cpp
REVS_PLAN_PRIVATE int chain_accept_impl(int32_t T, const double *s0, const double *s1, double scale, double eps,
                                        int32_t amax, int32_t kadd, int32_t chain_few, int32_t *nsup_sum,
                                        int32_t *nsup_max, int *why);                     // plan_newton.cpp
REVS_PLAN_PRIVATE int fold_alloc(revs_plan_t *plan);                                      // plan_fold.cpp

// ---- steps the native loops share ----------------------------------------------------------
// Scale of the voltage rows: max(|vlo|, |vhi|), never zero.
static inline double plan_scale(const revs_plan_desc_t &d) {
    return std::max(std::max(std::fabs(d.vlo), std::fabs(d.vhi)), 1e-300);
}

// The feeder's tree form as the C ABI's revs_tree_t.
static inline revs_tree_t plan_tree(const revs_plan *plan) {
    return revs_tree_t{plan->tree.n, (const uint64_t *)plan->tree.pack, plan->tree.w};
}

// The part of a sweep's call that no launch of a run changes; the loops set the rotating buffers per launch.
static inline revs::SweepCall plan_sweep_call(const revs_plan_desc_t &d, void *stream) {
    revs::SweepCall c;
    c.n_homes = d.n_homes; c.T = d.T;
    c.cost = d.cost; c.homes = d.homes; c.load = d.load;
    c.dsq = d.dsq; c.status = d.status;
    c.kappa = (float)d.kappa; c.mode = d.mode; c.pdhg = &d.pdhg;
    c.node_of = d.node_of;
    c.stream = stream;
    return c;
}

// Candidate set k (0 or 1) of the plan's descriptor: the lists, the stats block and its pinned host side.
struct PlanSet {
    int64_t *ci;
    int32_t *cc;
    double *cv, *st;
    const double *st_host;
};
static inline PlanSet plan_set(const revs_plan_desc_t &d, int k) {
    return k == 0 ? PlanSet{d.cand_idx, d.cand_cnt, d.cand_val, d.stats, d.stats_host}
                  : PlanSet{d.cand_idx1, d.cand_cnt1, d.cand_val1, d.stats1, d.stats1_host};
}

// Home pass of an evaluation of multipliers y into d.pnq and p_est_new: row-wise from the lists of set `sup`
// (use_y and sup >= 0: few multipliers, shifts straight from their rows of R, no dense product), else phase 1 of
// the evaluation kernel.  A sharded caller all-reduces d.pnq behind it.
static inline int plan_home_pass(const revs_plan_desc_t &d, const float *p_est, const float *p_sch, const float *gamma,
                                 const double *y, int use_y, int sup, float *p_est_new, void *stream) {
    if (use_y && sup >= 0) {
        const PlanSet S = plan_set(d, sup);
        return revs_op_dual_eval_rows(d.m, d.T, d.node_ptr, p_est, p_sch, gamma, d.R, S.ci, S.cc, y, d.kappa, d.pnq,
                                      p_est_new, stream);
    }
    return revs_op_dual_evaluate(1, d.m, d.T, d.node_ptr, p_est, p_sch, gamma, d.R, d.Rt, y, use_y, d.kappa, d.vlo, d.vhi,
                                 d.kadd, d.ksplit, d.d_slabs, d.v_slabs, d.pnq, p_est_new, d.vfull, d.viol, d.partial,
                                 d.cand_idx, d.cand_cnt, d.cand_val, d.stats, 0.0, nullptr, stream);
}

// Wait for an evaluation, not the launch: poll the sequence tag its selection writes into every slot's record of
// the pinned stats block `st` (lower latency than an event wait), then the acquire fence.  `who` names the entry
// point in the error text, `what` the thing waited for; t0: when the wait started.
static inline int wait_tags(const volatile double *st, int32_t T, double tag, hipStream_t s, const char *who,
                            const char *what,
                            std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now()) {
    for (int t = 0; t < T; ++t) {
        unsigned spins = 0;
        while (st[8 * t + 5] != tag) {
            if ((++spins & 0xFFFF) == 0) {
                if (hipStreamQuery(s) == hipSuccess && st[8 * t + 5] != tag) {
                    revs::set_error("%s: stream idle but stats tag missing", who);
                    return REVS_ELAUNCH;
                }
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) {
                    (void)hipStreamSynchronize(s);   // nothing of ours may still be writing
                    revs::set_error("%s: timed out waiting for %s", who, what);
                    return REVS_ELAUNCH;
                }
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return REVS_OK;
}

// The fields every folded-chain operator launch (revs::ChainKv) of a plan sets alike; the caller adds its sides,
// the model's pivot counts, the step's outputs and what is cleared on the way.
static inline revs::ChainKv chain_kv_common(const revs_plan *plan, double scale) {
    const revs_plan_desc_t &d = plan->d;
    revs::ChainKv c{};
    c.m = d.m; c.T = d.T; c.kadd = d.kadd;
    c.tree = plan->tree;
    c.vlo = d.vlo; c.vhi = d.vhi; c.kappa = d.kappa; c.delta = d.delta; c.scale = scale; c.eps = d.eps;
    c.max_pivots = d.max_pivots;
    c.R = d.R; c.k_full = d.k_full; c.yhat = d.yhat;
    c.sh_a = plan->fold_sh[0]; c.sh_b = plan->fold_sh[1];
    return c;
}
