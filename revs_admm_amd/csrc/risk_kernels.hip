// The voltage risk report (include/revs_admm_ops.h, "risk report"): per node and slot the standard
// deviation of the voltage drop under forecast error -- independent errors of variance s2 at the rows and up to two
// shared factors with loadings beta_k --, the margin z in standard deviations, the probability of a drop beyond drop_max
// and the drop that is exceeded with probability p_max.  drop = R g is linear, so
//     Var(drop[j]) = sum_i R[j][i]^2 s2[i] + sum_k ((R beta_k)[j])^2
// and with R[j][i] = wc[lca(i, j)] the first term is the path sum over j's ancestors-or-self a of w2[a] Q[a], Q the
// subtree sums of s2 and w2[a] = wc[a]^2 - wc[parent(a)]^2 = w[a] (2 wc[a] - w[a]) (feeder.risk_weights): the two scans
// every tree report opens with, on other inputs.
//
//   revs_net_risk   net_risk_kernel<NT, IPT>, the four shapes of tree_shape(), on revs_net_study's T x S grid; then
//                   risk_summary_kernel (one workgroup per (slot, scenario): box_select64 of boxplot.h over the staged
//                   secure drops) and risk_day_kernel (one thread per (scenario, position))
//
// One workgroup per (slot, scenario), 2 + K pairs of scans from net_scans.h's pieces, one after the other on the same LDS:
//   1. var_ind: net_gather of node_var (with its test, and a negative variance), net_flow_scan, net_times_w with w2 in
//      place of w, net_path_scan, the clamp at 0 -- kept in registers (skipped without node_var: +0.0);
//   2. per factor k: the drop's own code path on node_common[k]; var = var + c c (product, then sum);
//   3. the drop itself on node_g: the network report's bits; the slot's one flag (__syncthreads_or);
//   4. a pair of positions at a time sd, z, drop_q and prob, the stores in the caller's order and the staged values by
//      position at once (a chunk's results collected first cost the 1024 x 8 shape 16 spilled registers and the
//      8-position shapes a wavefront a SIMD), the counts, this thread's subtree of `expected`, its candidates for z_min
//      and sd_max;
//   5. the fixed tree above the threads (losses_kernels.hip's), the arg-min of z in (z up, caller index up) order with the
//      sd and the drop at it carried along, sd_max, the counts by LDS atomics, the slot record.
// Between two scans no barrier is added: net_path_scan's last reads of the buffer lie in front of the barrier inside the
// next net_flow_scan's block_excl_offset, its first write of the buffer behind it.
//
// LDS: the scans' buffer and wave totals (tree_lds_bytes) and, behind them, kRiskRedDoubles doubles for the reductions.
// The caller's scratch holds, by position, the staged drop_q, prob and z [S][T][n] each.
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"
#include "net_scans.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

struct RiskArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const double *var;            // variances of their independent errors double[S][m][T], or NULL
    const double *common;         // loadings of the shared factors double[K][S][m][T], or NULL (K == 0)
    const double *w2;             // per position: w (2 wc - w)
    const uint8_t *limit;         // per position, or NULL (every position with a row)
    const uint8_t *out_mask;      // per position, or NULL (every position)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t S, m, T, n_out, K;
    int32_t P;                    // threads that hold leaves of the fixed tree: next_pow2(n) / IPT (at least 1)
    double drop_max, z_max;
    double *sd, *z, *prob, *dropq, *drop;     // [S][n_out][T], or NULL
    revs_risk_slot_t *slot;       // [S][T], or NULL
    double *stage_q, *stage_p, *stage_z;      // [S][T][n] by position, or NULL
};

constexpr int kRiskRedDoubles = 6 * 16;     // the wave roots of expected; the arg-min's -z, sd and drop; sd_max; the arg-min's
                                            // indices (16 ints) and the two counts
inline size_t risk_lds_bytes(int n) { return (tree_lds_doubles_even(n) + kRiskRedDoubles) * sizeof(double); }

// (-z, index, sd, drop) in the arg-min's order: the smaller z, then the lower index; index -1: none
__device__ __forceinline__ void risk_better(double &bv, int &bi, double &bs, double &bd, double ov, int oi, double os, double od) {
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; bs = os; bd = od; }
}

// (net_scans.h above is compiled as every tree report compiles it: the drop keeps the network report's bits.)
// Everything below rounds each operation on its own (the contract's IEEE operations): no product is fused into a sum.
#pragma clang fp contract(off)

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void net_risk_kernel(RiskArgs A0) {
    extern __shared__ double risk_lds[];
    double *lds = risk_lds;
    RiskArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y, lane = tid & 63, wave = tid >> 6;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T, cell = ((int64_t)sc * T + t) * n, rows = (int64_t)sc * A.m * T;
        A.g += rows;
        if (A.var) A.var += rows;
        if (A.common) A.common += rows;
        if (A.sd) A.sd += arr;
        if (A.z) A.z += arr;
        if (A.prob) A.prob += arr;
        if (A.dropq) A.dropq += arr;
        if (A.drop) A.drop += arr;
        if (A.stage_q) { A.stage_q += cell; A.stage_p += cell; A.stage_z += cell; }
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *sred = lds + net_lds_doubles<NT, IPT>();               // [16] each: expected's wave roots,
    double *zred = sred + 16, *sat = zred + 16, *dat = sat + 16;    //   the arg-min's -z, the sd and the drop at it,
    double *smax = dat + 16;                                        //   sd_max
    int *ired = reinterpret_cast<int *>(smax + 16);                 // [16]
    int *cnt = ired + 16;                                           // n_risky, n_det
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (tid == 0) {
        lds[1] = 0.0;                                               // base[-1]
        cnt[0] = cnt[1] = 0;
    }

    double a[IPT], v[IPT];                                          // v: the variance of the drop
    bool bad = false;
    // ---- var_ind = the path sums of w2 Q, Q the subtree sums of the rows' variances
    if (A.var) {                                                    // (uniform)
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.var, A.m, A.T, t, act, se, a, &bad);
#pragma unroll
        for (int i = 0; i < IPT; ++i) bad |= a[i] < 0.0;
        net_flow_scan<NT, IPT>(act, lds, se, a);
        TreeArgs t2 = tr;
        t2.w = A.w2;
        net_times_w<IPT>(t2, act, jl, a);
        net_path_scan<NT, IPT>(tr, act, jl, lds, a);
#pragma unroll
        for (int i = 0; i < IPT; ++i) v[i] = a[i] > 0.0 ? a[i] : 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < IPT; ++i) v[i] = 0.0;
    }
    NET_CHUNK_FENCE();
    // ---- the shared factors: c_k = R beta_k by the drop's code path; var = var + c_k c_k
#pragma unroll 1
    for (int k = 0; k < A.K; ++k) {
        const double *beta = A.common + (int64_t)k * A.S * A.m * T;
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(beta, A.m, A.T, t, act, se, a, &bad);
        net_flow_scan<NT, IPT>(act, lds, se, a);
        net_times_w<IPT>(tr, act, jl, a);
        net_path_scan<NT, IPT>(tr, act, jl, lds, a);
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const double cc = a[i] * a[i];
            v[i] = v[i] + cc;
        }
        NET_CHUNK_FENCE();
    }
    // ---- the drop: the network report's scans
    {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, &bad);     // (A's fields, not locals: net_scans.h)
        net_flow_scan<NT, IPT>(act, lds, se, a);
    }
    NET_CHUNK_FENCE();
    net_times_w<IPT>(tr, act, jl, a);
    net_path_scan<NT, IPT>(tr, act, jl, lds, a);
    const bool badslot = __syncthreads_or(bad ? 1 : 0) != 0;        // (its barrier: every read of F is done)

    // ---- sd, z, drop_q, prob; the stores; the counts; this thread's subtree of expected and its candidates
    double half[IPT / kNetChunk];
    double bv = 0.0, bs = 0.0, bd = 0.0, sm = -inf;
    int bi = -1, n_risky = 0, n_det = 0;
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long lm = net_limit_bytes(tr, A.limit, jl + c);
        const unsigned long long om = net_load_bytes(A.out_mask, jl + c);
        double l1 = 0.0, l2 = 0.0;                                  // the pair tree's pending nodes: one per level
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 2) {                    // (a pair at a time, stored at once: nothing of a chunk
            double xs[2], xz[2], xq[2], xp[2], leaf[2];             //  is held beside the 2 IPT doubles of drop and var)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double d = a[c + i + e];
                const double sd = sqrt(v[c + i + e]);             // (correctly rounded, as network_kernels.hip's voltages)
                const double slack = A.drop_max - d;
                const double zz = sd > 0.0 ? slack / sd : (slack >= 0.0 ? inf : -inf);
                const double zs = A.z_max * sd;
                const double dq = d + zs;
                const double arg = zz * 0.70710678118654752;
                const double pr = 0.5 * erfc(arg);
                const bool cov = !badslot && nd[i + e] >= 0 && ((lm >> (8 * (i + e))) & 0xFFull) != 0ull &&
                                 ((om >> (8 * (i + e))) & 0xFFull) != 0ull;
                xs[e] = badslot ? nan : sd; xz[e] = badslot ? nan : zz;
                xq[e] = badslot ? nan : dq; xp[e] = badslot ? nan : pr;
                leaf[e] = cov ? pr : 0.0;
                n_risky += (cov && zz < A.z_max) ? 1 : 0;
                n_det += (cov && d > A.drop_max) ? 1 : 0;
                if (cov) {
                    risk_better(bv, bi, bs, bd, -zz, nd[i + e], sd, d);
                    sm = fmax(sm, sd);
                }
                if (nd[i + e] >= 0) {
                    const int64_t at = (int64_t)nd[i + e] * T + t;
                    if (A.drop) A.drop[at] = d;
                    if (A.sd) A.sd[at] = xs[e];
                    if (A.z) A.z[at] = xz[e];
                    if (A.prob) A.prob[at] = xp[e];
                    if (A.dropq) A.dropq[at] = xq[e];
                }
            }
            if (A.stage_q && act) {
                *reinterpret_cast<TreeD2 *>(A.stage_q + j0 + c + i) = TreeD2{{xq[0], xq[1]}};
                *reinterpret_cast<TreeD2 *>(A.stage_p + j0 + c + i) = TreeD2{{xp[0], xp[1]}};
                *reinterpret_cast<TreeD2 *>(A.stage_z + j0 + c + i) = TreeD2{{xz[0], xz[1]}};
            }
            const double pair = leaf[0] + leaf[1];
            if ((i & 2) == 0) { l1 = pair; continue; }
            const double quad = l1 + pair;
            if ((i & 4) == 0) l2 = quad;
            else half[c / kNetChunk] = l2 + quad;
        }
        NET_CHUNK_FENCE();
    }
    if (!A.slot) return;                                            // (uniform)
    double root;
    if constexpr (IPT == kNetChunk) root = half[0];
    else root = half[0] + half[IPT / kNetChunk - 1];
    // ---- the fixed tree above the threads: lanes by an xor butterfly, then the wavefronts' roots level by level
    const int P = A.P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if (o < P) root += __shfl_xor(root, o);                     // (uniform)
        n_risky += __shfl_xor(n_risky, o); n_det += __shfl_xor(n_det, o);
        const double ov = __shfl_xor(bv, o), os = __shfl_xor(bs, o), od = __shfl_xor(bd, o);
        const int oi = __shfl_xor(bi, o);
        risk_better(bv, bi, bs, bd, ov, oi, os, od);
        sm = fmax(sm, __shfl_xor(sm, o));
    }
    const int W = P > 64 ? P / 64 : 1;
    if (lane == 0) {
        if (wave < W) sred[wave] = root;
        zred[wave] = bv; ired[wave] = bi; sat[wave] = bs; dat[wave] = bd; smax[wave] = sm;
        if (n_risky) atomicAdd(cnt + 0, n_risky);
        if (n_det) atomicAdd(cnt + 1, n_det);
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = W; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) sred[i] = sred[2 * i] + sred[2 * i + 1];
        bv = zred[0]; bi = ired[0]; bs = sat[0]; bd = dat[0]; sm = smax[0];
        for (int w = 1; w < NT / 64; ++w) {
            risk_better(bv, bi, bs, bd, zred[w], ired[w], sat[w], dat[w]);
            sm = fmax(sm, smax[w]);
        }
        revs_risk_slot_t r;
        r.expected = badslot ? nan : sred[0];
        r.z_min = bi >= 0 ? -bv : nan;
        r.sd_at = bi >= 0 ? bs : nan;
        r.drop_at = bi >= 0 ? bd : nan;
        r.sd_max = bi >= 0 ? sm : nan;
        r.n_risky = cnt[0]; r.n_det = cnt[1];
        r.z_min_index = bi;
        r.n_bad = badslot ? 1 : 0;
        r.reserved[0] = r.reserved[1] = 0;
        A.slot[(size_t)sc * T + t] = r;
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged secure drops over the limit positions with
// out_mask and a caller-side index
constexpr int kRiskSumNT = 256;
struct RiskSumArgs {
    const double *stage;          // drop_q [S][T][n]
    const unsigned long long *pack;
    const uint8_t *limit;         // per position, or NULL (every position with a row)
    const uint8_t *mask;          // out_mask per position, or NULL
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T]
    int32_t T, n, n_out;
    double drop_max;
};

__global__ __launch_bounds__(kRiskSumNT) void risk_summary_kernel(RiskSumArgs A) {
    __shared__ BoxSelect<kRiskSumNT> sh;
    constexpr int NT = kRiskSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf();
    // box_select64's walk: an element is part of the sample when it is a summarised limit position and no NaN
    auto walk = [&](auto f) {
        net_for_each<NT>(row, A.n, A.nop, A.n_out, A.mask, [&](double v, int nd, int j) {
            if (nd >= 0 && !(A.limit ? A.limit[j] != 0 : (A.pack[j] & 0xFFFFull) != 0ull)) nd = -1;
            f(box_key(v), nd >= 0 && v == v, v, 0, nd);
        });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, above drop_max
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        if (ok) {
            s[2] += v > A.drop_max ? 1.0 : 0.0;
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
    revs_net_summary_t *out = A.out + (size_t)sc * A.T + t;
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    // ---- the selection; in its neighbour walk the worst node: the lowest caller-side index with the largest secure drop
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

// ---- the day of one (scenario, node) over the slots that are not bad (a bad slot's staged values are NaNs): the largest
// probability and its earliest slot, the smallest margin, the slots at risk, the expected number of slots below the limit
struct RiskDayArgs {
    const double *stage_p, *stage_z;  // [S][T][n]
    const int32_t *nop;
    revs_risk_day_t *out;             // [S][n_out]
    int32_t S, T, n, n_out;
    double z_max;
};

__global__ void risk_day_kernel(RiskDayArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.S * A.n) return;
    const int sc = idx / A.n, j = idx - sc * A.n;
    const int nd = A.nop ? A.nop[j] : j;
    if (nd < 0 || nd >= A.n_out) return;
    revs_risk_day_t r;
    r.prob_max = __builtin_nan(""); r.z_min = __builtin_nan(""); r.expected_slots = 0.0; r.prob_max_slot = -1; r.n_risky = 0;
    for (int t = 0; t < A.T; ++t) {
        const int64_t at = ((int64_t)sc * A.T + t) * A.n + j;
        const double p = A.stage_p[at], z = A.stage_z[at];
        if (p != p) continue;                     // (a bad slot is left out)
        if (r.prob_max_slot < 0 || z < r.z_min) r.z_min = z;
        if (r.prob_max_slot < 0 || p > r.prob_max) { r.prob_max = p; r.prob_max_slot = t; }
        r.n_risky += z < A.z_max ? 1 : 0;
        r.expected_slots = r.expected_slots + p;
    }
    A.out[(int64_t)sc * A.n_out + nd] = r;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_risk_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (!net_scratch_sizes_ok(S, T, tree_n)) return 0;
    return (int64_t)S * T * tree_n * 3 * (int64_t)sizeof(double);
}

extern "C" int revs_net_risk(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const revs_headroom_aux_t *aux,
                             const double *node_g, const double *node_var, const double *node_common, int32_t K,
                             const double *w2, const uint8_t *limit_mask, const uint8_t *out_mask, const int32_t *node_of_pos,
                             int32_t n_out, double drop_max, double z_max, double *sd_out, double *z_out, double *prob_out,
                             double *drop_q_out, double *drop_out, revs_risk_slot_t *slot_out, revs_net_summary_t *summary_out,
                             revs_risk_day_t *day_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_risk_slot_t) == 64 && sizeof(revs_risk_day_t) == 32, "");
    const char *who = "revs_net_risk";
    TreeArgs tr;
    int rc = net_tree_checks(who, S, m, T, tree, node_g, " node_g", n_out, &tr);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(aux && aux->parent_pos && aux->wc, "%s: null aux, aux->parent_pos or aux->wc", who);
    REVS_REQUIRE(aux->n_jump >= 0 && aux->n_jump <= REVS_HEADROOM_MAX_JUMP, "%s: aux->n_jump=%d outside 0..%d", who,
                 (int)aux->n_jump, REVS_HEADROOM_MAX_JUMP);
    REVS_REQUIRE(aux->n_jump == 0 || aux->jump, "%s: aux->jump is NULL with n_jump > 0", who);
    REVS_REQUIRE(drop_max - drop_max == 0.0, "%s: drop_max is not finite", who);
    REVS_REQUIRE(K >= 0 && K <= REVS_RISK_MAX_COMMON, "%s: K=%d outside 0..%d", who, (int)K, REVS_RISK_MAX_COMMON);
    REVS_REQUIRE(K == 0 || node_common, "%s: node_common is NULL with K > 0", who);
    REVS_REQUIRE(w2, "%s: null pointer argument w2", who);
    REVS_REQUIRE(z_max - z_max == 0.0 && z_max >= 0.0, "%s: z_max must be finite and >= 0", who);
    REVS_REQUIRE(sd_out || z_out || prob_out || drop_q_out || drop_out || slot_out || summary_out || day_out,
                 "%s: every output is NULL", who);
    const bool staged = summary_out || day_out;
    rc = net_scratch_checks(who, staged, scratch, "summary_out / day_out need", "revs_net_risk_scratch");
    if (rc != REVS_OK) return rc;
    const size_t cells = (size_t)S * T * tr.n;
    RiskArgs A;
    A.tr = tr;
    A.g = node_g; A.var = node_var; A.common = K > 0 ? node_common : nullptr; A.w2 = w2;
    A.limit = limit_mask; A.out_mask = out_mask; A.nop = node_of_pos;
    A.S = S; A.m = m; A.T = T; A.n_out = n_out; A.K = K; A.P = net_leaf_threads(tr.n);
    A.drop_max = drop_max; A.z_max = z_max;
    A.sd = sd_out; A.z = z_out; A.prob = prob_out; A.dropq = drop_q_out; A.drop = drop_out;
    A.slot = slot_out;
    A.stage_q = staged ? (double *)scratch : nullptr;
    A.stage_p = staged ? A.stage_q + cells : nullptr;
    A.stage_z = staged ? A.stage_q + 2 * cells : nullptr;
    rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        return launch_lds(net_risk_kernel<nt(), ipt()>, dim3(T, S), dim3(nt()), risk_lds_bytes(tr.n), (hipStream_t)stream, who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out) {
        RiskSumArgs P;
        P.stage = A.stage_q; P.pack = tr.pack; P.limit = limit_mask; P.mask = out_mask; P.nop = node_of_pos;
        P.out = summary_out; P.T = T; P.n = tr.n; P.n_out = n_out; P.drop_max = drop_max;
        hipLaunchKernelGGL(risk_summary_kernel, dim3(T, S), dim3(kRiskSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        RiskDayArgs D;
        D.stage_p = A.stage_p; D.stage_z = A.stage_z; D.nop = node_of_pos; D.out = day_out;
        D.S = S; D.T = T; D.n = tr.n; D.n_out = n_out; D.z_max = z_max;
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(risk_day_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, D);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
