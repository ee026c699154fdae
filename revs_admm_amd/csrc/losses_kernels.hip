// The loss report (include/revs_admm_ops.h, "loss report"): per line and slot the power the
// feeder loses carrying a schedule, per node the marginal loss factor, per slot and per day the sums and what they cost.
//
//   revs_net_losses   net_losses_kernel<NT, IPT>, the four shapes of tree_shape(), on revs_net_study's T x S grid; then
//                     loss_summary_kernel (one workgroup per (slot, scenario), box_select64 of boxplot.h over the staged
//                     losses), loss_line_day_kernel (one thread per (scenario, position)) and loss_day_kernel (one
//                     workgroup per scenario: the slot loops and the top 8 by repeated arg-max)
//
// One workgroup per (slot, scenario):
//   1. the flow and the drop scans of the network report (net_scans.h; between the gather and the flow scan each thread
//      takes the pair-tree sum of its gathered injections): the same bits;
//   2. den = vset2 - drop, and the slot's one flag: a row's injection not finite, or den > 0 failing where the position
//      has a caller-side index (one __syncthreads_or);
//   3. loss = ((0.5 w) flow) flow / den and c = (w flow) / den in registers, the losses stored and staged by position;
//   4. mlf = net_path_scan(c): the sum of c over the ancestors-or-self, in the drop scan's form;
//   5. the sums -- total, delivered, class_total[4] -- as the root of ONE fixed binary tree over the positions: pairs
//      inside the thread's aligned 8 (16) positions, an xor butterfly over the lanes, then the wavefronts' roots level by
//      level in LDS; only the next_pow2(n) / IPT threads that hold leaves take part, so no padding zero is ever added
//      above the root;
//   6. the largest mlf and the lowest caller-side index that has it (lanes, then wavefronts).
// The 1024 x 16 shape has 128 registers per thread: it does not carry the flows through the drop scan but runs the flow
// scan again behind it (the same bits: its order is fixed), as net_headroom_kernel does.
//
// LDS: the scans' buffer and wave totals (tree_lds_bytes) and, behind them, kLossRedDoubles doubles for the sums and the
// arg-max.  The caller's scratch holds the staged losses [S][T][n], the slot records [S][T] and the lines' day energies
// [S][n] that the later launches read.
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"       // pair_tree, arg_better, wave_argmax
#include "net_scans.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

struct LossArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const uint8_t *line_mask;     // per position, or NULL (every line)
    const uint8_t *node_mask;     // per position, or NULL (every node)
    const uint8_t *line_class;    // per position, or NULL (C == 0)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t m, T, n_out, C;
    int32_t P;                    // threads that hold leaves of the fixed tree: next_pow2(n) / IPT (at least 1)
    double vset2;
    double *loss, *mlf;           // [S][n_out][T], or NULL
    double *drop, *flow;          // [S][n_out][T], or NULL
    revs_loss_slot_t *slot;       // [S][T], or NULL
    revs_loss_slot_t *slot_scr;   // [S][T] in the scratch, or NULL
    double *stage;                // [S][T][n] by position, or NULL
};

constexpr int kLossSums = 6;       // delivered, total, class_total[4]
constexpr int kLossRedDoubles = kLossSums * 16 + 16 + 8;      // the sums' wave roots, the arg-max's values and indices

inline size_t loss_lds_bytes(int n) { return (tree_lds_doubles_even(n) + kLossRedDoubles) * sizeof(double); }

// (net_scans.h above is compiled as every tree report compiles it: flow and drop keep the network report's bits.)
// Everything below rounds each operation on its own (the contract's IEEE operations): no product is fused into a sum.
#pragma clang fp contract(off)

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void net_losses_kernel(LossArgs A0) {
    extern __shared__ double loss_lds[];
    double *lds = loss_lds;
    LossArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T;
        A.g += (int64_t)sc * A.m * T;
        if (A.loss) A.loss += arr;
        if (A.mlf) A.mlf += arr;
        if (A.drop) A.drop += arr;
        if (A.flow) A.flow += arr;
        if (A.stage) A.stage += ((int64_t)sc * T + t) * n;
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *sred = lds + net_lds_doubles<NT, IPT>();               // [kLossSums][16]
    double *mred = sred + kLossSums * 16;                           // [16]
    int *ired = reinterpret_cast<int *>(mred + 16);                 // [16]
    constexpr bool kRescan = IPT > 8;
    const double nan = __builtin_nan("");
    if (tid == 0) lds[1] = 0.0;                                     // base[-1]

    double a[IPT], f[IPT];                                          // f: the flows (kRescan: from the second flow scan)
    double root[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // this thread's subtree of each sum
    bool bad = false;
    {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, &bad);     // (A's fields, not locals: net_scans.h)
        root[0] = pair_tree<IPT>(a);
        net_flow_scan<NT, IPT>(act, lds, se, a);
    }
    NET_CHUNK_FENCE();
    // ---- flow out
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        if (A.flow) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.flow[(int64_t)nd[i] * T + t] = a[c + i];
        }
        if constexpr (!kRescan) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) f[c + i] = a[c + i];
        }
        NET_CHUNK_FENCE();
    }
    // ---- drop = the path sums of w flow; den = vset2 - drop; the slot's flag
    net_times_w<IPT>(tr, act, jl, a);
    net_path_scan<NT, IPT>(tr, act, jl, lds, a);
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) {
            if (A.drop && nd[i] >= 0) A.drop[(int64_t)nd[i] * T + t] = a[c + i];
            a[c + i] = A.vset2 - a[c + i];
            bad |= nd[i] >= 0 && !(a[c + i] > 0.0);
        }
        NET_CHUNK_FENCE();
    }
    const bool badslot = __syncthreads_or(bad ? 1 : 0) != 0;        // (its barrier: every read of F is done)
    if constexpr (kRescan) {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, f, nullptr);
        net_flow_scan<NT, IPT>(act, lds, se, f);
    }
    // ---- loss and c per line; the losses out and staged; this thread's subtrees of total and class_total
    double half[IPT / kNetChunk][kLossSums - 1];
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long lm = net_load_bytes(A.line_mask, jl + c);
        const unsigned long long lc = A.line_class ? net_load_bytes(A.line_class, jl + c) : ~0ull;
        double x[kNetChunk];
        double l1[kLossSums - 1], l2[kLossSums - 1];                // the pair tree's pending nodes: one per level
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 2) {
            const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + jl + c + i);
            double leaf[2][kLossSums - 1];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double w = wv.v[e], fl = f[c + i + e], den = a[c + i + e];
                const double ls = act ? ((0.5 * w) * fl) * fl / den : 0.0;
                a[c + i + e] = act ? (w * fl) / den : 0.0;                          // c
                x[i + e] = badslot ? nan : ls;
                const bool summed = nd[i + e] >= 0 && ((lm >> (8 * (i + e))) & 0xFFull) != 0ull;
                leaf[e][0] = summed ? ls : 0.0;
                const int k = (int)((lc >> (8 * (i + e))) & 0xFFull);
#pragma unroll
                for (int q = 0; q < 4; ++q) leaf[e][1 + q] = (act && k == q && q < A.C) ? ls : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kLossSums - 1; ++q) {
                const double pair = leaf[0][q] + leaf[1][q];
                if ((i & 2) == 0) { l1[q] = pair; continue; }
                const double quad = l1[q] + pair;
                if ((i & 4) == 0) l2[q] = quad;
                else half[c / kNetChunk][q] = l2[q] + quad;
            }
        }
        if (A.loss) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.loss[(int64_t)nd[i] * T + t] = x[i];
        }
        if (A.stage && act) {
#pragma unroll
            for (int i = 0; i < kNetChunk; i += 2) *reinterpret_cast<TreeD2 *>(A.stage + j0 + c + i) = TreeD2{{x[i], x[i + 1]}};
        }
        NET_CHUNK_FENCE();
    }
#pragma unroll
    for (int q = 0; q < kLossSums - 1; ++q) {
        if constexpr (IPT == kNetChunk) root[1 + q] = half[0][q];
        else root[1 + q] = half[0][q] + half[IPT / kNetChunk - 1][q];
    }
    // ---- mlf = the path sums of c (every read of the buffer is done: the flag's barrier, or the second flow scan's)
    net_path_scan<NT, IPT>(tr, act, jl, lds, a);
    double bv = 0.0;
    int bi = -1;
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        const unsigned long long nm = net_load_bytes(A.node_mask, jl + c);
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) {
            const double v = badslot ? nan : a[c + i];
            if (A.mlf && nd[i] >= 0) A.mlf[(int64_t)nd[i] * T + t] = v;
            if (((nm >> (8 * i)) & 0xFFull) != 0ull && v == v) arg_better(bv, bi, v, nd[i]);
        }
        NET_CHUNK_FENCE();
    }
    if (!A.slot && !A.slot_scr) return;                             // (uniform)
    // ---- the fixed tree above the threads: lanes by an xor butterfly, then the wavefronts' roots level by level
    const int P = A.P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if (o < P) {                                                // (uniform)
#pragma unroll
            for (int q = 0; q < kLossSums; ++q) root[q] += __shfl_xor(root[q], o);
        }
    }
    wave_argmax(bv, bi);
    const int lane = tid & 63, wave = tid >> 6, W = P > 64 ? P / 64 : 1;
    if (lane == 0) {
        if (wave < W) {
#pragma unroll
            for (int q = 0; q < kLossSums; ++q) sred[q * 16 + wave] = root[q];
        }
        mred[wave] = bv; ired[wave] = bi;
    }
    __syncthreads();
    if (tid < kLossSums) {
        double *r = sred + tid * 16;
        for (int w = W; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    } else if (tid == 64) {
        double v = mred[0];
        int ix = ired[0];
        for (int w = 1; w < NT / 64; ++w) arg_better(v, ix, mred[w], ired[w]);
        mred[0] = v; ired[0] = ix;
    }
    __syncthreads();
    if (tid == 0) {
        revs_loss_slot_t r;
        r.delivered = badslot ? nan : sred[0];
        r.total = badslot ? nan : sred[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) r.class_total[q] = badslot ? nan : (q < A.C ? sred[(2 + q) * 16] : 0.0);
        const int ix = badslot ? -1 : ired[0];
        r.mlf_max = ix >= 0 ? mred[0] : nan;
        r.mlf_max_index = ix;
        r.n_bad = badslot ? 1 : 0;
        if (A.slot) A.slot[(size_t)sc * T + t] = r;
        if (A.slot_scr) A.slot_scr[(size_t)sc * T + t] = r;
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged losses over the lines with line_mask
constexpr int kLossSumNT = 256;
struct LossSumArgs {
    const double *stage;          // [S][T][n]
    const uint8_t *mask;          // line_mask per position, or NULL
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T]
    int32_t T, n, n_out;
    double loss_max;
};

__global__ __launch_bounds__(kLossSumNT) void loss_summary_kernel(LossSumArgs A) {
    __shared__ BoxSelect<kLossSumNT> sh;
    constexpr int NT = kLossSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf();
    // box_select64's walk: an element is part of the sample when it is summarised and no NaN
    auto walk = [&](auto f) {
        net_for_each<NT>(row, A.n, A.nop, A.n_out, A.mask, [&](double v, int nd, int) { f(box_key(v), nd >= 0 && v == v, v, 0, nd); });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, above loss_max
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        if (ok) {
            s[2] += v > A.loss_max ? 1.0 : 0.0;
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
    // ---- the selection; in its neighbour walk the worst line: the lowest caller-side index with the largest loss
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

// ---- the day of one (scenario, line): the energy lost, the largest loss and its earliest slot; the energy by position
// into the scratch for the day kernel's top 8
__global__ void loss_line_day_kernel(const double *stage, const int32_t *nop, revs_loss_line_day_t *out, double *energy_scr,
                                     int S, int T, int n, int n_out, double slot_hours) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * n) return;
    const int sc = idx / n, j = idx - sc * n;
    double acc = 0.0, peak = 0.0;
    int at = -1;
    bool anynan = false;
    for (int t = 0; t < T; ++t) {
        const double v = stage[((int64_t)sc * T + t) * n + j];
        acc = acc + v;
        anynan |= v != v;
        if (at < 0 || v > peak) { peak = v; at = t; }
    }
    revs_loss_line_day_t r;
    r.energy = acc * slot_hours;
    r.peak = anynan ? __builtin_nan("") : peak;
    r.peak_slot = anynan ? -1 : at;
    r.reserved = 0;
    energy_scr[(int64_t)sc * n + j] = r.energy;
    const int nd = nop ? nop[j] : j;
    if (out && nd >= 0 && nd < n_out) out[(int64_t)sc * n_out + nd] = r;
}

// ---- the day of one scenario: the slot records summed in slot order by one thread, then the eight summarised lines of
// largest day energy by eight arg-max rounds, each over the lines after the last pick in (energy down, index up) order
constexpr int kLossDayNT = 256;
struct LossDayArgs {
    const revs_loss_slot_t *slot; // [S][T]
    const double *energy;         // [S][n] by position
    const uint8_t *mask;          // line_mask per position, or NULL
    const int32_t *nop;
    const double *cost;           // [T], or NULL
    revs_loss_day_t *out;         // [S]
    int32_t T, n, n_out;
    double slot_hours;
};

__global__ __launch_bounds__(kLossDayNT) void loss_day_kernel(LossDayArgs A) {
    __shared__ double mv[kLossDayNT / 64];
    __shared__ int mi[kLossDayNT / 64];
    __shared__ revs_loss_day_t rec;
    const int tid = threadIdx.x, sc = (int)blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nan = __builtin_nan("");
    if (tid == 0) {
        const revs_loss_slot_t *s = A.slot + (size_t)sc * A.T;
        double e = 0.0, d = 0.0, ce[4] = {0.0, 0.0, 0.0, 0.0}, co = 0.0, peak = 0.0;
        int at = -1, nbad = 0;
        for (int t = 0; t < A.T; ++t) {
            const double tot = s[t].total;
            e = e + tot; d = d + s[t].delivered;
            for (int q = 0; q < 4; ++q) ce[q] = ce[q] + s[t].class_total[q];
            if (A.cost) { const double pr = tot * A.cost[t]; co = co + pr; }
            if (at < 0 || tot > peak) { peak = tot; at = t; }
            nbad += s[t].n_bad;
        }
        rec.energy = e * A.slot_hours; rec.delivered = d * A.slot_hours;
        for (int q = 0; q < 4; ++q) rec.class_energy[q] = ce[q] * A.slot_hours;
        rec.cost = A.cost ? co * A.slot_hours : nan;
        rec.peak = nbad ? nan : peak; rec.peak_slot = nbad ? -1 : at;
        rec.n_bad_slots = nbad;
        for (int q = 0; q < 6; ++q) rec.reserved[q] = 0;
    }
    const double *en = A.energy + (size_t)sc * A.n;
    double pv = __builtin_inf();
    int pi = -1;                                   // the last pick: everything is after (+inf, -1)
    for (int k = 0; k < 8; ++k) {
        double bv = 0.0;
        int bi = -1;
        for (int j = tid; j < A.n; j += kLossDayNT) {
            int nd = A.nop ? A.nop[j] : j;
            nd = (nd >= 0 && nd < A.n_out && (!A.mask || A.mask[j] != 0)) ? nd : -1;
            const double v = en[j];
            if (nd >= 0 && v == v && (v < pv || (v == pv && nd > pi))) arg_better(bv, bi, v, nd);
        }
        wave_argmax(bv, bi);
        if (lane == 0) { mv[wave] = bv; mi[wave] = bi; }
        __syncthreads();
        bv = mv[0]; bi = mi[0];
        for (int w = 1; w < kLossDayNT / 64; ++w) arg_better(bv, bi, mv[w], mi[w]);
        __syncthreads();                           // (every read of mv / mi is done)
        if (tid == 0) { rec.top_index[k] = bi; rec.top_energy[k] = bi >= 0 ? bv : nan; }
        if (bi >= 0) { pv = bv; pi = bi; }
        else { pv = -__builtin_inf(); pi = 0x7FFFFFFF; }       // (uniform) nothing is left
    }
    if (tid == 0) A.out[sc] = rec;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_losses_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (!net_scratch_sizes_ok(S, T, tree_n)) return 0;
    return (int64_t)S * T * tree_n * (int64_t)sizeof(double) + (int64_t)S * T * (int64_t)sizeof(revs_loss_slot_t) +
           (int64_t)S * tree_n * (int64_t)sizeof(double);
}

extern "C" int revs_net_losses(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                               const uint8_t *line_mask, const uint8_t *node_mask, const uint8_t *line_class, int32_t C,
                               const int32_t *node_of_pos, int32_t n_out, double vset2, double slot_hours, double loss_max,
                               const double *cost, double *loss_out, double *mlf_out, double *drop_out, double *flow_out,
                               revs_net_summary_t *summary_out, revs_loss_slot_t *slot_out, revs_loss_line_day_t *line_day_out,
                               revs_loss_day_t *day_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_loss_slot_t) == 64 && sizeof(revs_loss_line_day_t) == 24 && sizeof(revs_loss_day_t) == 192, "");
    const char *who = "revs_net_losses";
    TreeArgs tr;
    int rc = net_tree_checks(who, S, m, T, tree, node_g, " node_g", n_out, &tr);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(vset2 - vset2 == 0.0 && vset2 > 0.0, "%s: vset2 must be finite and > 0", who);
    REVS_REQUIRE(slot_hours - slot_hours == 0.0 && slot_hours > 0.0, "%s: slot_hours must be finite and > 0", who);
    REVS_REQUIRE(loss_max > 0.0, "%s: loss_max must be > 0 (+inf allowed)", who);
    REVS_REQUIRE(C >= 0 && C <= 4, "%s: C=%d outside 0..4", who, (int)C);
    REVS_REQUIRE(C == 0 || line_class, "%s: line_class is NULL with C > 0", who);
    REVS_REQUIRE(loss_out || mlf_out || drop_out || flow_out || summary_out || slot_out || line_day_out || day_out,
                 "%s: every output is NULL", who);
    const bool staged = summary_out || line_day_out || day_out;
    rc = net_scratch_checks(who, staged, scratch, "summary_out / line_day_out / day_out need", "revs_net_losses_scratch");
    if (rc != REVS_OK) return rc;
    double *stage = staged ? (double *)scratch : nullptr;
    revs_loss_slot_t *slot_scr = staged ? (revs_loss_slot_t *)(stage + (size_t)S * T * tr.n) : nullptr;
    double *energy_scr = staged ? (double *)(slot_scr + (size_t)S * T) : nullptr;
    LossArgs A;
    A.tr = tr;
    A.g = node_g; A.line_mask = line_mask; A.node_mask = node_mask; A.line_class = C > 0 ? line_class : nullptr;
    A.nop = node_of_pos;
    A.m = m; A.T = T; A.n_out = n_out; A.C = C; A.vset2 = vset2; A.P = net_leaf_threads(tr.n);
    A.loss = loss_out; A.mlf = mlf_out; A.drop = drop_out; A.flow = flow_out;
    A.slot = slot_out; A.slot_scr = day_out ? slot_scr : nullptr;
    A.stage = stage;
    rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        return launch_lds(net_losses_kernel<nt(), ipt()>, dim3(T, S), dim3(nt()), loss_lds_bytes(tr.n), (hipStream_t)stream, who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out) {
        LossSumArgs P;
        P.stage = stage; P.mask = line_mask; P.nop = node_of_pos; P.out = summary_out;
        P.T = T; P.n = tr.n; P.n_out = n_out; P.loss_max = loss_max;
        hipLaunchKernelGGL(loss_summary_kernel, dim3(T, S), dim3(kLossSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (line_day_out || day_out) {
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(loss_line_day_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double *)stage, node_of_pos, line_day_out, energy_scr, (int)S, (int)T, (int)tr.n, (int)n_out,
                           slot_hours);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        LossDayArgs D;
        D.slot = slot_scr; D.energy = energy_scr; D.mask = line_mask; D.nop = node_of_pos; D.cost = cost; D.out = day_out;
        D.T = T; D.n = tr.n; D.n_out = n_out; D.slot_hours = slot_hours;
        hipLaunchKernelGGL(loss_day_kernel, dim3(S), dim3(kLossDayNT), 0, (hipStream_t)stream, D);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
