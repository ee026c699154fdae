// librevs_admm.so's error reporting, version string and LDS grants; the plan's lifecycle, setters, timing and
// status word.  The native loops that drive a plan are in plan_newton.cpp, plan_fold.cpp and plan_stream.cpp.
#include "plan.h"
#include <stdarg.h>
#include <map>
#include <mutex>

namespace revs {
bool grant_lds(const void *kernel, size_t bytes, const char *who) {
    if (bytes <= 64 * 1024) return true;
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    size_t &g = granted[{kernel, dev}];
    if (g >= bytes) return true;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        set_error("%s: %zu bytes of LDS refused: %s", who, bytes, hipGetErrorString(e));
        return false;
    }
    g = bytes;
    return true;
}
}  // namespace revs

namespace revs {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace revs

extern "C" const char *revs_last_error(void) { return revs::g_err; }
extern "C" const char *revs_version(void) { return "revs_admm_amd 0.1 (gfx950)"; }

// Device-side address of pinned host memory (hipHostMalloc / torch pin_memory): lets a
// kernel write its few result words where the host reads them, without a copy kernel.
extern "C" int revs_host_device_ptr(void *host_ptr, void **dev_ptr) {
    REVS_REQUIRE(host_ptr && dev_ptr, "revs_host_device_ptr: null argument");
    const hipError_t e = hipHostGetDevicePointer(dev_ptr, host_ptr, 0);
    if (e != hipSuccess) {
        revs::set_error("revs_host_device_ptr: %s", hipGetErrorString(e));
        return REVS_EINVAL;
    }
    return REVS_OK;
}

extern "C" revs_plan_t *revs_plan_create(const revs_plan_desc_t *desc) {
    if (!desc || !desc->stats || !desc->stats_host || !desc->pnq || desc->T <= 0 || desc->m <= 0) {
        revs::set_error("revs_plan_create: bad descriptor");
        return nullptr;
    }
    revs_plan *p = new revs_plan{*desc, nullptr, 0.0, nullptr};
    const size_t nb = sizeof(uint32_t) * ((desc->m + 31) / 32);
    hipError_t e = hipEventCreateWithFlags(&p->ev, hipEventDisableTiming);
    const char *what = "hipEventCreateWithFlags";
    if (e == hipSuccess) { e = hipMalloc((void **)&p->counters, nb); what = "hipMalloc"; }
    if (e == hipSuccess) { e = hipMemset(p->counters, 0, nb); what = "hipMemset"; }
    if (e != hipSuccess) {
        revs::set_error("revs_plan_create: %s: %s", what, hipGetErrorString(e));
        if (p->ev) (void)hipEventDestroy(p->ev);
        if (p->counters) (void)hipFree(p->counters);
        delete p;
        return nullptr;
    }
    // control block, record ring and status word of the streaming steady state
    const revs::StreamCtl ctl0{0u, 0u, 0ull};
    void *host = nullptr;
    what = "hipMalloc";
    e = hipMalloc((void **)&p->ctl, sizeof(revs::StreamCtl));
    if (e == hipSuccess) { e = hipMemcpy(p->ctl, &ctl0, sizeof(ctl0), hipMemcpyHostToDevice); what = "hipMemcpy"; }
    if (e == hipSuccess) {
        e = hipHostMalloc(&host, sizeof(double) * 4 * revs::kRecRing + 64, hipHostMallocMapped);
        what = "hipHostMalloc";
    }
    if (e == hipSuccess) {
        p->rec_host = (double *)host;
        p->flags_host = (unsigned int *)(p->rec_host + 4 * revs::kRecRing);
        for (int i = 0; i < 4 * revs::kRecRing; ++i) p->rec_host[i] = -1.0;
        *p->flags_host = 0u;
        void *dp = nullptr;
        e = hipHostGetDevicePointer(&dp, host, 0);
        what = "hipHostGetDevicePointer";
        p->rec_dev = (double *)dp;
        p->flags_dev = (unsigned int *)(p->rec_dev + 4 * revs::kRecRing);
    }
    if (e != hipSuccess) {
        revs::set_error("revs_plan_create: %s: %s", what, hipGetErrorString(e));
        revs_plan_destroy(p);
        return nullptr;
    }
    (void)plan_wg_order(p);       // (here, not inside the first burst: a copy of the residence records to the host and a sort)
    return p;
}

// The order in which a multi-iteration sweep's launch takes its workgroups of residences: those that hold the most
// residences with an EV first (a residence without one has no QP to solve: its wavefront runs a third of the
// instructions).  A launch of 100 000 residences is 3 125 workgroups on a chip that holds 1 280 at a time: its last round
// cannot fill the chip, and with the heavy workgroups in front that round is made of the quick ones.  Nothing else
// changes: the same workgroups do the same work (node sums are exact: order-independent).  NULL when the descriptor
// carries no residence records (then: launch order = residence order).
const int32_t *plan_wg_order(revs_plan_t *plan) {
    if (plan->wg_order_tried) return plan->wg_order;
    plan->wg_order_tried = true;
#ifdef REVS_TUNING        // (tuning builds: A/B of the order inside one job)
    if (getenv("REVS_NO_WG_ORDER")) return nullptr;
#endif
    const revs_plan_desc_t &d = plan->d;
    const int64_t per = revs::agent_homes_per_block(d.T, d.pdhg.lanes);
    if (!d.homes || d.n_homes <= 0 || per <= 0) return nullptr;
    const int64_t nb = (d.n_homes + per - 1) / per;
    if (nb < 2 || nb >= (1ll << 31)) return nullptr;
    std::vector<revs_home_t> h((size_t)d.n_homes);
    if (hipMemcpy(h.data(), d.homes, sizeof(revs_home_t) * (size_t)d.n_homes, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
    std::vector<int32_t> w((size_t)nb, 0), order((size_t)nb);
    for (int64_t i = 0; i < d.n_homes; ++i) w[(size_t)(i / per)] += h[(size_t)i].ev != 0;
    for (int64_t b = 0; b < nb; ++b) order[(size_t)b] = (int32_t)b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return w[(size_t)x] > w[(size_t)y]; });
    if (hipMalloc((void **)&plan->wg_order, sizeof(int32_t) * (size_t)nb) != hipSuccess) { plan->wg_order = nullptr; return nullptr; }
    if (hipMemcpy(plan->wg_order, order.data(), sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(plan->wg_order);
        plan->wg_order = nullptr;
    }
    return plan->wg_order;
}

extern "C" void revs_plan_destroy(revs_plan_t *plan) {
    if (!plan) return;
    if (plan->wg_order) (void)hipFree(plan->wg_order);
    if (plan->ev) (void)hipEventDestroy(plan->ev);
    if (plan->counters) (void)hipFree(plan->counters);
    if (plan->ctl) (void)hipFree(plan->ctl);
    if (plan->rec_host) (void)hipHostFree(plan->rec_host);
    if (plan->ring) (void)hipFree(plan->ring);
    if (plan->grp_bits) (void)hipFree(plan->grp_bits);
    if (plan->grp_dmax) (void)hipFree(plan->grp_dmax);
    for (int i = 0; i < 2; ++i) {
        if (plan->fold_e2[i]) (void)hipFree(plan->fold_e2[i]);      // (fold_e1[i ^ 1] is its second half)
        if (plan->fold_ci[i]) (void)hipFree(plan->fold_ci[i]);
        if (plan->fold_cc[i]) (void)hipFree(plan->fold_cc[i]);
        if (plan->fold_cv[i]) (void)hipFree(plan->fold_cv[i]);
        if (plan->fold_st_host[i]) (void)hipHostFree(plan->fold_st_host[i]);
    }
    for (double *v : plan->fold_v) if (v) (void)hipFree(v);
    for (double *v : plan->fold_st_local) if (v) (void)hipFree(v);
    for (int32_t *v : plan->fold_info) if (v) (void)hipFree(v);
    for (double *v : plan->fold_sh) if (v) (void)hipFree(v);
    for (hipEvent_t e : plan->events) (void)hipEventDestroy(e);
    for (hipEvent_t e : plan->tev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : plan->cev) if (e) (void)hipEventDestroy(e);
    if (plan->side) (void)hipStreamDestroy(plan->side);
    delete plan;
}

extern "C" int revs_plan_set_tree(revs_plan_t *plan, const revs_tree_t *t) {
    REVS_REQUIRE(plan, "revs_plan_set_tree: null plan");
    if (!t || t->n == 0) { plan->tree = revs::TreeArgs{}; return REVS_OK; }
    const revs::TreeArgs tr = revs::tree_args(t);
    REVS_REQUIRE(revs::tree_form_ok(tr), "revs_plan_set_tree: " REVS_TREE_FORM_MSG, REVS_TREE_FORM_ARGS(tr, REVS_TREE_MAX));
    plan->tree = tr;
    return REVS_OK;
}

extern "C" int revs_plan_set_comm(revs_plan_t *plan, revs_comm_t *comm) {
    REVS_REQUIRE(plan, "revs_plan_set_comm: null plan");
    plan->comm = comm;
    return REVS_OK;
}

extern "C" int revs_plan_set_stream_block(revs_plan_t *plan, int32_t block, int32_t overlap) {
    REVS_REQUIRE(plan && block >= 0 && block <= REVS_STREAM_BLOCK_MAX,
                 "revs_plan_set_stream_block: block=%d outside 0..%d", block, REVS_STREAM_BLOCK_MAX);
    if (block <= 1) { plan->block = 0; return REVS_OK; }
    const revs_plan_desc_t &d = plan->d;
    REVS_REQUIRE(d.n_homes > 0 && d.node_of, "revs_plan_set_stream_block: the plan has no residences / node_of");
    REVS_REQUIRE(d.recompute_pe_new, "revs_plan_set_stream_block: verdicts by blocks need recompute_pe_new");
    if (!plan->grp_bits) {
        const size_t gb = sizeof(unsigned long long) * (REVS_STREAM_BLOCK_MAX + 4);   // (+ the call's first iteration, + the handed-over slice)
        hipError_t e = hipMalloc((void **)&plan->grp_bits, 2 * gb);                    // (maxima, then the slices' arrival words)
        if (e == hipSuccess) e = hipMemset(plan->grp_bits, 0, 2 * gb);
        if (e == hipSuccess) e = hipMalloc((void **)&plan->grp_dmax, gb);
        if (e == hipSuccess) e = hipMemset(plan->grp_dmax, 0, gb);
        if (e == hipSuccess && !plan->side) e = hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking);
        if (e != hipSuccess) {
            revs::set_error("revs_plan_set_stream_block: %s", hipGetErrorString(e));
            plan->block = 0;
            return REVS_ELAUNCH;
        }
    }
    plan->block = block;
    plan->overlap = overlap != 0;
    return REVS_OK;
}

// Everything the run loops would otherwise allocate the first time they need it: the ring of node-sum slices and the
// event pool of the block form (for the block size, stream count and communicator the plan has NOW -- a later
// change is picked up by the loops as before), the folded chain's buffers.  A fresh engine's first run then makes no
// allocation, no synchronising memset and no event between its launches (round 5: ~0.5 ms of a 2.2 ms transient).
extern "C" int revs_plan_prepare(revs_plan_t *plan) {
    REVS_REQUIRE(plan, "revs_plan_prepare: null plan");
    const revs_plan_desc_t &d = plan->d;
    if (d.cand_idx1 && d.stats1_host && plan->tree.n > 0) {
        const int rc = fold_alloc(plan);
        if (rc != REVS_OK) return rc;
    }
    if (plan->block > 1 && d.n_homes > 0) {
        const int nranks = plan->comm ? plan->comm->nranks : 1;
        const size_t stride = (size_t)d.m * d.T + (size_t)REVS_DMAX_SLOTS * nranks;
        const size_t need = (size_t)2 * plan->block * stride;
        hipError_t e = hipSuccess;
        if (plan->ring_cap < need) {
            if (plan->ring) { (void)hipDeviceSynchronize(); (void)hipFree(plan->ring); }
            plan->ring = nullptr;
            plan->ring_cap = 0;
            e = hipMalloc((void **)&plan->ring, sizeof(double) * need);
            if (e == hipSuccess) plan->ring_cap = need;
        }
        if (e == hipSuccess && plan->ring_dirty) {
            e = hipMemset(plan->ring, 0, sizeof(double) * plan->ring_cap);
            if (e == hipSuccess) plan->ring_dirty = false;
        }
        while (e == hipSuccess && plan->events.size() < 2 * 8 + 1) {      // (a burst of eight blocks: 256 iterations)
            hipEvent_t ev;
            e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e == hipSuccess) plan->events.push_back(ev);
        }
        if (e != hipSuccess) {
            revs::set_error("revs_plan_prepare: %s", hipGetErrorString(e));
            return REVS_ELAUNCH;
        }
    }
    return REVS_OK;
}

extern "C" int revs_plan_set_kadd_cold(revs_plan_t *plan, int32_t kadd_cold, int32_t cold_at) {
    REVS_REQUIRE(plan && kadd_cold >= 0 && kadd_cold <= 64 && cold_at >= 0, "revs_plan_set_kadd_cold: kadd_cold=%d (0..64), cold_at=%d", kadd_cold, cold_at);
    plan->kadd_cold = kadd_cold;
    plan->kadd_cold_at = cold_at;
    return REVS_OK;
}

extern "C" int revs_plan_set_fold_redo(revs_plan_t *plan, int32_t steps) {
    REVS_REQUIRE(plan && steps >= 0 && steps <= 8, "revs_plan_set_fold_redo: steps=%d outside 0..8", steps);
    plan->fold_redo = steps;
    return REVS_OK;
}

extern "C" int revs_plan_set_stream_inner(revs_plan_t *plan, int32_t inner) {
    REVS_REQUIRE(plan && inner >= 1 && inner <= REVS_AGENT_MAX_INNER,
                 "revs_plan_set_stream_inner: inner=%d outside 1..%d", inner, REVS_AGENT_MAX_INNER);
    plan->inner = inner;
    return REVS_OK;
}

extern "C" int revs_plan_set_pdhg_dual(revs_plan_t *plan, float *pdhg_dual) {
    REVS_REQUIRE(plan && (pdhg_dual != nullptr) == (plan->d.pdhg_dual != nullptr),
                 "revs_plan_set_pdhg_dual: the plan was created %s carried multipliers",
                 plan && plan->d.pdhg_dual ? "with" : "without");
    plan->d.pdhg_dual = pdhg_dual;
    return REVS_OK;
}

extern "C" int revs_plan_stream_timing(revs_plan_t *plan, int32_t enable) {
    REVS_REQUIRE(plan, "revs_plan_stream_timing: null plan");
    for (hipEvent_t &e : plan->tev)
        if (enable && !e && hipEventCreate(&e) != hipSuccess) {
            revs::set_error("revs_plan_stream_timing: hipEventCreate failed");
            return REVS_ELAUNCH;
        }
    for (hipEvent_t &e : plan->cev)
        if (enable && plan->comm && !e && hipEventCreate(&e) != hipSuccess) {
            revs::set_error("revs_plan_stream_timing: hipEventCreate failed");
            return REVS_ELAUNCH;
        }
    plan->timing = enable ? 1 : 0;
    plan->cev_valid = false;
    return REVS_OK;
}

extern "C" int revs_plan_collective_ms(revs_plan_t *plan, double *collective_ms, double *block_ms, int32_t *iterations) {
    REVS_REQUIRE(plan && collective_ms && block_ms && iterations, "revs_plan_collective_ms: null argument");
    REVS_REQUIRE(plan->cev_valid, "revs_plan_collective_ms: no block's all-reduce has been timed (one GPU, or revs_plan_stream_timing not armed)");
    float a = 0.f, b = 0.f;
    hipError_t e = hipEventElapsedTime(&a, plan->cev[0], plan->cev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&b, plan->cev[2], plan->cev[3]);
    if (e != hipSuccess) {
        revs::set_error("revs_plan_collective_ms: %s (synchronise the streams first)", hipGetErrorString(e));
        return REVS_ELAUNCH;
    }
    *collective_ms = (double)a;
    *block_ms = (double)b;
    *iterations = plan->cev_nb;
    return REVS_OK;
}

extern "C" int revs_plan_stream_elapsed_ms(revs_plan_t *plan, double *ms) {
    REVS_REQUIRE(plan && ms, "revs_plan_stream_elapsed_ms: null argument");
    REVS_REQUIRE(plan->timing == 2, "revs_plan_stream_elapsed_ms: no burst since revs_plan_stream_timing");
    float f = 0.f;
    const hipError_t e = hipEventElapsedTime(&f, plan->tev[0], plan->tev[1]);
    if (e != hipSuccess) {
        revs::set_error("revs_plan_stream_elapsed_ms: %s (synchronise the stream first)", hipGetErrorString(e));
        return REVS_ELAUNCH;
    }
    *ms = (double)f;
    plan->timing = 1;
    return REVS_OK;
}

extern "C" int64_t revs_plan_stream_launches(revs_plan_t *plan) {
    return plan ? plan->timed_launches : 0;
}

extern "C" int32_t revs_plan_status_flags(revs_plan_t *plan, int32_t clear) {
    if (!plan || !plan->flags_host) return 0;
    const unsigned int f = *(volatile unsigned int *)plan->flags_host;
    if (clear) *(volatile unsigned int *)plan->flags_host = 0u;
    return (int32_t)f;
}
