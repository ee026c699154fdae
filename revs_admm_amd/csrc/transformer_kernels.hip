// The transformer report (include/revs_admm_ops.h, "transformer report"): per service transformer
// and slot the load, the load ratio, the top-oil and hot-spot temperatures and the ageing factor of a schedule, per
// transformer and day the peaks, the energy and the loss of insulation life, per slot the box-plot records over the
// fleet, per scenario the fleet's sums and the eight transformers that age most.
//
//   revs_xf_report   xf_report_kernel, one workgroup per tile of kXfTile transformers of one scenario; then
//                    xf_summary_kernel (one workgroup per (slot, scenario, quantity), box_select64 of boxplot.h over the
//                    staged ratios / hot-spots) and xf_fleet_kernel (one workgroup per scenario: the fixed-tree sums over
//                    the day records and the top 8 by repeated arg-max, fixed_tree.h)
//
// One workgroup of xf_report_kernel:
//   A. all threads, cells (transformer, slot) with the slot fastest so that the rows of g are read in pieces: the grouped
//      sum in list order, the ratio, the two ultimate rises (the two pow); load and ratio go out as they are formed (the
//      tile's transformers are one contiguous piece of [S][K][T]); u_to, u_w, ratio and |load| are staged in LDS as
//      [slot][transformer], a row of kXfTile + 1 doubles (the odd row length keeps a wavefront's 8-byte accesses along
//      the slots on distinct banks); a bad member, rating or row index sets the transformer's flag in LDS;
//   B. one thread per transformer: the cyclic start's pass (no exp), then the real pass over the slots and sub-steps in
//      place -- u_to becomes top_oil, u_w hot_spot, |load| faa -- and the day record;
//   C. all threads: the three arrays out with the slot fastest, the ratios and hot-spots into the scratch as
//      [S][T][K] with the transformer fastest, which xf_summary_kernel reads coalesced.
// LDS: 4 T (kXfTile + 1) doubles + kXfTile flags: 102 KB at T = 192 (tiles of 64 would need 400 KB).  Tiles of 32 and 64
// where they fit (T <= 96, T <= 48) were measured and are slower by 1.3 - 1.7: phase B keeps one
// wavefront of a workgroup busy, and with small tiles several workgroups share a compute unit's LDS meanwhile.
//
// Everything in this file rounds each operation on its own (the contract's IEEE operations): no product is fused into a
// sum.  pow and exp are the device library's.
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"
#include "tree_body.h"        // launch_lds

#include <math.h>

#pragma clang fp contract(off)

namespace revs {

constexpr int kXfTile = 16;                       // transformers of one workgroup
constexpr int kXfPad = kXfTile + 1;               // doubles per LDS row
constexpr int kXfNT = 256;

struct XfArgs {
    const double *g;              // node sums double[S][m][T]
    const int32_t *ptr, *rows;    // CSR: [K + 1], [nnz]
    const double *rated;          // [K]
    const double *ambient;        // [T]
    revs_xf_model_t mdl;
    double slot_hours, decay_to, decay_w, to0, w0, over_ratio, hot_limit;
    int32_t m, T, K, nnz, q, cyclic;
    double *load, *ratio, *top_oil, *hot, *faa;   // [S][K][T], or NULL
    double *st_ratio, *st_hot;    // [S][T][K] in the scratch, or NULL
    revs_xf_day_t *day;           // [S][K], or NULL
};

inline size_t xf_lds_bytes(int T) { return (size_t)4 * T * kXfPad * sizeof(double) + kXfTile * sizeof(int); }

__global__ __launch_bounds__(kXfNT) void xf_report_kernel(XfArgs A) {
    extern __shared__ __attribute__((aligned(16))) double xf_lds[];
    const int tid = threadIdx.x, sc = (int)blockIdx.y, k0 = (int)blockIdx.x * kXfTile, T = A.T;
    const int nk = A.K - k0 < kXfTile ? A.K - k0 : kXfTile, cells = nk * T;
    double *uto = xf_lds, *uw = uto + T * kXfPad, *rat = uw + T * kXfPad, *abl = rat + T * kXfPad;
    int *badf = reinterpret_cast<int *>(abl + T * kXfPad);
    const double nan = __builtin_nan("");
    if (tid < kXfTile) badf[tid] = 0;
    __syncthreads();
    const double *g = A.g + (int64_t)sc * A.m * T;
    const int64_t arr = ((int64_t)sc * A.K + k0) * T;              // the tile's piece of an [S][K][T] array
    // ---- A: the grouped sums and the ultimate rises
    const double R = A.mdl.loss_ratio, r1 = R + 1.0;
    for (int idx = tid; idx < cells; idx += kXfNT) {
        const int kl = idx / T, t = idx - kl * T, k = k0 + kl;
        int p0 = A.ptr[k], p1 = A.ptr[k + 1];
        p0 = p0 < 0 ? 0 : p0; p1 = p1 > A.nnz ? A.nnz : p1;        // (never outside xf_rows)
        double load = 0.0;
        bool bad = false;
        for (int j = p0; j < p1; ++j) {
            const int row = A.rows[j];
            if (row >= 0 && row < A.m) {                           // (never outside g)
                const double v = g[(int64_t)row * T + t];
                load = load + v;
                bad |= !(v - v == 0.0);
            } else {
                bad = true;
            }
        }
        const double rk = A.rated[k];
        bad |= !(rk - rk == 0.0 && rk > 0.0);
        const double al = fabs(load), ratio = al / rk, r2 = ratio * ratio;
        const int at = t * kXfPad + kl;
        uto[at] = A.mdl.dto_r * pow((r2 * R + 1.0) / r1, A.mdl.n);
        uw[at] = A.mdl.dhs_r * pow(r2, A.mdl.m);
        rat[at] = ratio; abl[at] = al;
        if (A.load) A.load[arr + idx] = load;
        if (A.ratio) A.ratio[arr + idx] = ratio;
        if (bad) atomicOr(badf + kl, 1);
    }
    __syncthreads();
    // ---- B: the recursion, one thread per transformer
    if (tid < nk) {
        const int kl = tid, q = A.q;
        const bool bad = badf[kl] != 0;
        const double dto = A.decay_to, dw = A.decay_w;
        double x = A.to0, y = A.w0;
        if (A.cyclic) {
            double aN = 1.0, awN = 1.0;
            x = 0.0; y = 0.0;
            for (int t = 0; t < T; ++t) {
                const double u1 = uto[t * kXfPad + kl], u2 = uw[t * kXfPad + kl];
                for (int s = 0; s < q; ++s) {
                    x = u1 + (x - u1) * dto; y = u2 + (y - u2) * dw;
                    aN = aN * dto; awN = awN * dw;
                }
            }
            x = x / (1.0 - aN); y = y / (1.0 - awN);
        }
        const double B = A.mdl.aging_B, c0 = B / (A.mdl.theta_ref + 273.0);
        double e = 0.0, age = 0.0, pr = nan, ph = nan;
        int prs = -1, phs = -1, nover = 0, nhot = 0;
        for (int t = 0; t < T; ++t) {
            const int at = t * kXfPad + kl;
            const double u1 = uto[at], u2 = uw[at], ratio = rat[at], al = abl[at], amb = A.ambient[t];
            double acc = 0.0, hot = nan;
            for (int s = 0; s < q; ++s) {
                x = u1 + (x - u1) * dto; y = u2 + (y - u2) * dw;
                hot = (amb + x) + y;
                acc = acc + exp(c0 - B / (hot + 273.0));
            }
            const double f = acc / (double)q;
            e = e + al; age = age + f;
            if (t == 0 || ratio > pr) { pr = ratio; prs = t; }
            if (t == 0 || hot > ph) { ph = hot; phs = t; }
            nover += ratio > A.over_ratio ? 1 : 0;
            nhot += hot > A.hot_limit ? 1 : 0;
            uto[at] = bad ? nan : x; uw[at] = bad ? nan : hot; abl[at] = bad ? nan : f;
        }
        if (A.day) {
            revs_xf_day_t r;
            const double ah = age * A.slot_hours;
            r.peak_ratio = bad ? nan : pr; r.peak_hot = bad ? nan : ph;
            r.energy_kwh = bad ? nan : e * A.slot_hours;
            r.age_hours = bad ? nan : ah;
            r.lol_percent = bad ? nan : 100.0 * ah / A.mdl.normal_life_hours;
            r.feqa = bad ? nan : ah / ((double)T * A.slot_hours);
            r.peak_ratio_slot = bad ? -1 : prs; r.peak_hot_slot = bad ? -1 : phs;
            r.n_over_slots = bad ? 0 : nover; r.n_hot_slots = bad ? 0 : nhot;
            A.day[(int64_t)sc * A.K + k0 + kl] = r;
        }
    }
    __syncthreads();
    // ---- C: the arrays out (slot fastest), the summaries' staging (transformer fastest)
    if (A.top_oil || A.hot || A.faa) {
        for (int idx = tid; idx < cells; idx += kXfNT) {
            const int kl = idx / T, t = idx - kl * T, at = t * kXfPad + kl;
            if (A.top_oil) A.top_oil[arr + idx] = uto[at];
            if (A.hot) A.hot[arr + idx] = uw[at];
            if (A.faa) A.faa[arr + idx] = abl[at];
        }
    }
    if (A.st_ratio) {
        for (int idx = tid; idx < cells; idx += kXfNT) {
            const int t = idx / nk, kl = idx - t * nk, at = t * kXfPad + kl;
            const int64_t to = ((int64_t)sc * T + t) * A.K + k0 + kl;
            A.st_ratio[to] = rat[at]; A.st_hot[to] = uw[at];
        }
    }
}

// ---- the summary of one (slot, scenario, quantity): the box-plot record over the K transformers
constexpr int kXfSumNT = 256;
struct XfSumArgs {
    const double *stage[2];       // [S][T][K]: ratios, hot-spots
    revs_net_summary_t *out[2];   // [S][T]
    double limit[2];              // over_ratio, hot_limit
    int32_t T, K, first;          // first: the quantity of blockIdx.z == 0
};

__global__ __launch_bounds__(kXfSumNT) void xf_summary_kernel(XfSumArgs A) {
    __shared__ BoxSelect<kXfSumNT> sh;
    constexpr int NT = kXfSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y, which = A.first + (int)blockIdx.z;
    const double *row = A.stage[which] + ((int64_t)sc * A.T + t) * A.K;
    const double limit = A.limit[which];
    const double ninf = -__builtin_inf();
    // box_select64's walk: a transformer is part of the sample when its value is no NaN; every thread the same trips
    auto walk = [&](auto f) {
        for (int jb = 0; jb < A.K; jb += NT) {
            const int j = jb + tid;
            const bool in = j < A.K;
            const double v = in ? row[j] : __builtin_nan("");
            f(box_key(v), in && v == v, v, 0, in ? j : -1);
        }
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, above the limit
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        if (ok) {
            s[2] += v > limit ? 1.0 : 0.0;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v);
        }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 3, true>(s, sh.red);
    block_reduce_multi<NT, 2, false>(x, sh.red);
    const int kcnt = (int)s[0];
    revs_net_summary_t r;
    const double nan = __builtin_nan("");
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.worst_value = nan;
    r.count = kcnt; r.n_fliers = 0; r.n_violations = (int)s[2]; r.n_nan = (int)s[1];
    r.worst_index = -1;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    revs_net_summary_t *out = A.out[which] + (size_t)sc * A.T + t;
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    double wi[1] = {ninf};
    const BoxFigures b = box_select64(sh, kcnt, walk, [&](unsigned long long, bool ok, double v, int, int nd) {
        if (ok && v == x[1]) wi[0] = fmax(wi[0], -(double)nd);
    });
    block_reduce_multi<NT, 1, false>(wi, sh.red);
    if (tid == 0) {
        r.min = -x[0]; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo; r.whisker_hi = b.whi;
        r.n_fliers = b.n_fliers;
        r.worst_value = x[1]; r.worst_index = (int)-wi[0];
        *out = r;
    }
}

// ---- the fleet of one scenario: counts, the three sums as roots of the fixed binary tree over the transformers -- 8 per
// thread, an xor butterfly over the lanes, the four wavefronts, 2048 transformers a round, the rounds' roots level by level
// (the values are >= +0.0 or NaN, so the zeros beyond K change no bit wherever the tree ends) -- and the top 8
constexpr int kXfFleetNT = 256;
constexpr int kXfRound = kXfFleetNT * 8;
constexpr int kXfRounds = 32;                     // 65536 / kXfRound
struct XfFleetArgs {
    const revs_xf_day_t *day;     // [S][K]
    revs_xf_fleet_t *out;         // [S]
    int32_t T, K;
    double slot_hours;
};

__global__ __launch_bounds__(kXfFleetNT) void xf_fleet_kernel(XfFleetArgs A) {
    constexpr int NT = kXfFleetNT;
    __shared__ double red[(NT / 64) * kBlockRed];
    __shared__ double wroot[3][NT / 64];
    __shared__ double sroot[3][kXfRounds];
    __shared__ double mv[NT / 64];
    __shared__ int mi[NT / 64];
    __shared__ revs_xf_fleet_t rec;
    const int tid = threadIdx.x, sc = (int)blockIdx.x, lane = tid & 63, wave = tid >> 6, K = A.K;
    const revs_xf_day_t *day = A.day + (size_t)sc * K;
    const double nan = __builtin_nan("");
    // ---- the counts
    double cnt[4] = {0.0, 0.0, 0.0, 0.0};         // NaN records, overloaded, hot, ageing
    for (int j = tid; j < K; j += NT) {
        const revs_xf_day_t d = day[j];
        cnt[0] += d.lol_percent != d.lol_percent ? 1.0 : 0.0;
        cnt[1] += d.n_over_slots > 0 ? 1.0 : 0.0;
        cnt[2] += d.n_hot_slots > 0 ? 1.0 : 0.0;
        cnt[3] += d.feqa > 1.0 ? 1.0 : 0.0;
    }
    block_reduce_multi<NT, 4, true>(cnt, red);
    // ---- the sums: lol_percent, energy_kwh, age_hours
    if (tid < 3 * kXfRounds) sroot[tid / kXfRounds][tid % kXfRounds] = 0.0;
    __syncthreads();
    const int rounds = (K + kXfRound - 1) / kXfRound;
    for (int c = 0; c < rounds; ++c) {
        double x[3][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = c * kXfRound + tid * 8 + i;
            const bool in = j < K;
            x[0][i] = in ? day[j].lol_percent : 0.0;
            x[1][i] = in ? day[j].energy_kwh : 0.0;
            x[2][i] = in ? day[j].age_hours : 0.0;
        }
        double r[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) r[e] = pair_tree<8>(x[e]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int e = 0; e < 3; ++e) r[e] += __shfl_xor(r[e], o);
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) wroot[e][wave] = r[e];
        }
        __syncthreads();
        if (tid < 3) sroot[tid][c] = (wroot[tid][0] + wroot[tid][1]) + (wroot[tid][2] + wroot[tid][3]);
        __syncthreads();
    }
    if (tid < 3) {
        double *r = sroot[tid];
        for (int w = kXfRounds; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    }
    __syncthreads();
    if (tid == 0) {
        rec.lol_sum = sroot[0][0]; rec.energy_kwh = sroot[1][0];
        rec.feqa_mean = sroot[2][0] / (((double)K * (double)A.T) * A.slot_hours);
        rec.n_xf = K; rec.n_nan = (int)cnt[0]; rec.n_overloaded = (int)cnt[1]; rec.n_hot = (int)cnt[2];
        rec.n_aging = (int)cnt[3];
        rec.reserved[0] = rec.reserved[1] = rec.reserved[2] = 0;
    }
    // ---- the top 8: arg-max rounds, each over the transformers after the last pick in (lol down, index up) order
    double pv = __builtin_inf();
    int pi = -1;
    for (int k = 0; k < 8; ++k) {
        double bv = 0.0;
        int bi = -1;
        for (int j = tid; j < K; j += NT) {
            const double v = day[j].lol_percent;
            if (v == v && (v < pv || (v == pv && j > pi))) arg_better(bv, bi, v, j);
        }
        wave_argmax(bv, bi);
        if (lane == 0) { mv[wave] = bv; mi[wave] = bi; }
        __syncthreads();
        bv = mv[0]; bi = mi[0];
        for (int w = 1; w < NT / 64; ++w) arg_better(bv, bi, mv[w], mi[w]);
        __syncthreads();                           // (every read of mv / mi is done)
        if (tid == 0) { rec.top_index[k] = bi; rec.top_lol[k] = bi >= 0 ? bv : nan; }
        if (bi >= 0) { pv = bv; pi = bi; }
        else { pv = -__builtin_inf(); pi = 0x7FFFFFFF; }       // (uniform) nothing is left
    }
    if (tid == 0) {
        rec.lol_max = rec.top_lol[0];
        A.out[sc] = rec;
    }
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_xf_report_scratch(int32_t S, int32_t T, int32_t K) {
    if (S < 1 || S > REVS_STUDY_MAX_S || T < 1 || T > REVS_MAX_T || K < 1 || K > 0xFFFF) return 0;
    return (int64_t)2 * S * T * K * (int64_t)sizeof(double) + (int64_t)S * K * (int64_t)sizeof(revs_xf_day_t);
}

static bool xf_finite(double v) { return v - v == 0.0; }

extern "C" int revs_xf_report(int32_t S, int32_t m, int32_t T, int32_t K, int32_t nnz, const double *node_g,
                              const int32_t *xf_ptr, const int32_t *xf_rows, const double *rated_kw, const double *ambient,
                              const revs_xf_model_t *model, double slot_hours, int32_t substeps, double decay_to,
                              double decay_w, int32_t cyclic, double to0, double w0, double over_ratio, double hot_limit,
                              double *load_out, double *ratio_out, double *top_oil_out, double *hot_out, double *faa_out,
                              revs_net_summary_t *sum_ratio_out, revs_net_summary_t *sum_hot_out, revs_xf_day_t *xf_day_out,
                              revs_xf_fleet_t *fleet_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_xf_model_t) == 64 && sizeof(revs_xf_day_t) == 64 && sizeof(revs_xf_fleet_t) == 160, "");
    const char *who = "revs_xf_report";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0 && m <= 0xFFFF, "%s: m=%d outside 1..65535", who, (int)m);
    REVS_REQUIRE(K > 0 && K <= 0xFFFF, "%s: K=%d outside 1..65535", who, (int)K);
    REVS_REQUIRE(nnz >= 0 && nnz <= m, "%s: nnz=%d outside 0..m", who, (int)nnz);
    REVS_REQUIRE(node_g, "%s: null pointer argument node_g", who);
    REVS_REQUIRE(xf_ptr, "%s: null pointer argument xf_ptr", who);
    REVS_REQUIRE(xf_rows || nnz == 0, "%s: null pointer argument xf_rows with nnz > 0", who);
    REVS_REQUIRE(rated_kw, "%s: null pointer argument rated_kw", who);
    REVS_REQUIRE(ambient, "%s: null pointer argument ambient", who);
    REVS_REQUIRE(model, "%s: null pointer argument model", who);
    const revs_xf_model_t M = *model;
    REVS_REQUIRE(xf_finite(M.dto_r) && M.dto_r > 0.0, "%s: model dto_r must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.dhs_r) && M.dhs_r > 0.0, "%s: model dhs_r must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.loss_ratio) && M.loss_ratio > 0.0, "%s: model loss_ratio must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.n) && M.n > 0.0, "%s: model n must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.m) && M.m > 0.0, "%s: model m must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.aging_B) && M.aging_B > 0.0, "%s: model aging_B must be finite and > 0", who);
    REVS_REQUIRE(xf_finite(M.theta_ref) && M.theta_ref > -273.0, "%s: model theta_ref must be finite and > -273", who);
    REVS_REQUIRE(xf_finite(M.normal_life_hours) && M.normal_life_hours > 0.0,
                 "%s: model normal_life_hours must be finite and > 0", who);
    REVS_REQUIRE(slot_hours - slot_hours == 0.0 && slot_hours > 0.0, "%s: slot_hours must be finite and > 0", who);
    REVS_REQUIRE(substeps >= 1 && substeps <= 16, "%s: substeps=%d outside 1..16", who, (int)substeps);
    REVS_REQUIRE(decay_to >= 0.0 && decay_to < 1.0, "%s: decay_to outside [0, 1)", who);
    REVS_REQUIRE(decay_w >= 0.0 && decay_w < 1.0, "%s: decay_w outside [0, 1)", who);
    REVS_REQUIRE(cyclic == 0 || cyclic == 1, "%s: cyclic=%d is neither 0 nor 1", who, (int)cyclic);
    REVS_REQUIRE(cyclic == 1 || (xf_finite(to0) && xf_finite(w0)), "%s: to0 and w0 must be finite with cyclic = 0", who);
    REVS_REQUIRE(over_ratio == over_ratio && hot_limit == hot_limit, "%s: over_ratio and hot_limit must be no NaN", who);
    REVS_REQUIRE(load_out || ratio_out || top_oil_out || hot_out || faa_out || sum_ratio_out || sum_hot_out || xf_day_out ||
                 fleet_out, "%s: every output is NULL", who);
    const bool staged = sum_ratio_out || sum_hot_out || fleet_out;
    REVS_REQUIRE(!staged || scratch, "%s: sum_ratio_out / sum_hot_out / fleet_out need scratch (revs_xf_report_scratch bytes)", who);
    REVS_REQUIRE(!staged || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    const bool sums = sum_ratio_out || sum_hot_out;
    double *st_ratio = sums ? (double *)scratch : nullptr;
    double *st_hot = sums ? st_ratio + (size_t)S * T * K : nullptr;
    revs_xf_day_t *day_scr = staged ? (revs_xf_day_t *)((double *)scratch + (size_t)2 * S * T * K) : nullptr;
    XfArgs A;
    A.g = node_g; A.ptr = xf_ptr; A.rows = xf_rows; A.rated = rated_kw; A.ambient = ambient;
    A.mdl = M;
    A.slot_hours = slot_hours; A.decay_to = decay_to; A.decay_w = decay_w; A.to0 = to0; A.w0 = w0;
    A.over_ratio = over_ratio; A.hot_limit = hot_limit;
    A.m = m; A.T = T; A.K = K; A.nnz = nnz; A.q = substeps; A.cyclic = cyclic;
    A.load = load_out; A.ratio = ratio_out; A.top_oil = top_oil_out; A.hot = hot_out; A.faa = faa_out;
    A.st_ratio = st_ratio; A.st_hot = st_hot;
    A.day = xf_day_out ? xf_day_out : (fleet_out ? day_scr : nullptr);
    const int rc = launch_lds(xf_report_kernel, dim3((K + kXfTile - 1) / kXfTile, S), dim3(kXfNT), xf_lds_bytes(T),
                              (hipStream_t)stream, who, A);
    if (rc != REVS_OK) return rc;
    if (sums) {
        XfSumArgs P;
        P.stage[0] = st_ratio; P.stage[1] = st_hot;
        P.out[0] = sum_ratio_out; P.out[1] = sum_hot_out;
        P.limit[0] = over_ratio; P.limit[1] = hot_limit;
        P.T = T; P.K = K; P.first = sum_ratio_out ? 0 : 1;
        hipLaunchKernelGGL(xf_summary_kernel, dim3(T, S, sum_ratio_out && sum_hot_out ? 2 : 1), dim3(kXfSumNT), 0,
                           (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (fleet_out) {
        XfFleetArgs F;
        F.day = A.day; F.out = fleet_out; F.T = T; F.K = K; F.slot_hours = slot_hours;
        hipLaunchKernelGGL(xf_fleet_kernel, dim3(S), dim3(kXfFleetNT), 0, (hipStream_t)stream, F);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
