// The voltage attribution report (include/revs_admm_ops.h, "attribution report"): per slot the
// watched node -- a given one, or the limit node of largest drop -- and per node how much of that node's drop its
// injection causes: contrib[i] = R[j*][i] inj[i] with R[j*][i] = wc[lca(i, j*)], the EV part of it, the sums by class,
// and how many nodes reach the watched one, carry a large share, or could clear its excess alone.
//
//   revs_net_attribution   net_attr_kernel<NT, IPT>, the four shapes of tree_shape(), on revs_net_study's T x S grid;
//                          then attr_summary_kernel (one workgroup per (slot, scenario): box_select64 of boxplot.h over
//                          the staged contributions, then the top 8 by repeated arg-max) and attr_day_kernel (one thread
//                          per (scenario, position))
//
// One workgroup per (slot, scenario):
//   1. the flow and the drop scans of the network report in this file's own text (net_scans.h's pieces restated:
//      attr_flow_scan is net_gather, with node_ev's test, and net_flow_scan; attr_path_scan its net_path_scan -- from
//      the pieces the kernel was up to 1.5% slower on a 30-scenario grid): the same bits;
//   2. the slot's one flag (a row's injection not finite: __syncthreads_or), the drops out, and the watched position:
//      the arg-max of drop over the limit positions in (drop down, caller index up) order, lanes then wavefronts;
//   3. sens[i] = wc[lca(i, j*)] without a walk.  The marked positions (a <= j* < end[a]) are j*'s root path and wc does
//      not decrease down it (w >= 0), so the deepest marked ancestor of i is the one of largest wc:
//        i <= j*:  the marked ancestors of i are the marked a <= i            -> inclusive prefix max of marked ? wc : 0
//        i >  j*:  the marked ancestors of i are the marked a with end[a] > i -> suffix max of wc[a] deposited at
//                  end[a] - 1 (an LDS atomic max; the bit patterns of doubles >= 0 order as unsigned integers)
//      Two block scans with max, three barriers: a selection, the same bits whichever way it is computed;
//   4. the products, one rounding each; the six sums as the root of ONE fixed binary tree (losses_kernels.hip's: pairs
//      inside the thread's aligned 8 (16) positions, an xor butterfly over the lanes, the wavefronts' roots level by level
//      in LDS); the integer counts by LDS atomics; the stores.
//
// LDS: the scans' buffer and wave totals (tree_lds_bytes) and, behind them, kAttrRedDoubles doubles for the sums, the
// arg-max and the slot's scalars.  The caller's scratch holds, by position, the staged contributions and EV contributions
// [S][T][n], the slot records [S][T] and one flag byte per cell [S][T][n] that the later launches read.
#include "common.h"
#include "boxplot.h"
#include "fixed_tree.h"       // arg_better, wave_argmax
#include "tree_body.h"

#include <math.h>

namespace revs {

struct AttrArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const double *ev;             // their EV part double[S][m][T], or NULL
    const double *wc;             // per position: the resistance (x 2) of the path from the substation
    const uint8_t *limit;         // per position, or NULL (every position with a row)
    const uint8_t *out_mask;      // per position, or NULL (every position)
    const uint8_t *cls;           // class_of_pos per position, or NULL (C == 0)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t m, T, n_out, C;
    int32_t P;                    // threads that hold leaves of the fixed tree: next_pow2(n) / IPT (at least 1)
    int32_t watch_pos;            // -1: the slot's worst limit position
    double drop_max, frac;
    double *sens, *contrib, *evc; // [S][n_out][T], or NULL
    double *drop;                 // [S][n_out][T], or NULL
    revs_attr_slot_t *slot;       // [S][T], or NULL
    revs_attr_slot_t *slot_scr;   // [S][T] in the scratch, or NULL
    double *stage, *stage_ev;     // [S][T][n] by position, or NULL
    uint8_t *flags;               // [S][T][n] by position, or NULL
};

constexpr int kAttrChunk = 8;      // positions whose side data are in flight at once (net_scans.h: kNetChunk)
constexpr int kAttrSums = 6;       // total, ev_total, class_total[4]
constexpr int kAttrRedDoubles = kAttrSums * 16 + 16 + 8 + 8 + 8;  // the sums' wave roots; the arg-max's values, indices and
                                                                  // positions; the slot's scalars
constexpr unsigned kAttrSummarised = 1u, kAttrReach = 2u, kAttrBig = 4u;      // the staged flag byte
#define ATTR_FENCE() __builtin_amdgcn_sched_barrier(0)

template <int NT, int IPT>
constexpr size_t attr_lds_doubles() { return (2 + (size_t)NT * IPT + 2 * (NT / 64) + 1) / 2 * 2; }
inline size_t attr_lds_bytes(int n) { return (tree_lds_doubles_even(n) + kAttrRedDoubles) * sizeof(double); }

// net_scans.h's net_gather and net_flow_scan in one, with one addition: bad |= a gathered EV node sum is not finite.
template <int NT, int IPT>
__device__ __forceinline__ void attr_flow_scan(const AttrArgs &A, int t, double *lds, const unsigned (&se)[IPT], double (&a)[IPT],
                                               bool &bad) {
    const int tid = threadIdx.x, j0 = IPT * tid;
    const bool act = j0 < A.tr.n;
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {          // (positions without a row fetch row 0: straight-line loads, masked behind them)
        const int s = (int)(se[i] & 0xFFFFu) - 1;
        const bool ok = act && s >= 0 && s < A.m;
        const double v = A.g[(int64_t)(ok ? s : 0) * A.T + t];
        a[i] = ok ? v : 0.0;
        bad |= !(a[i] - a[i] == 0.0);
    }
    if (A.ev) {
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int s = (int)(se[i] & 0xFFFFu) - 1;
            const bool ok = act && s >= 0 && s < A.m;
            const double v = A.ev[(int64_t)(ok ? s : 0) * A.T + t];
            bad |= ok && !(v - v == 0.0);
        }
    }
#pragma unroll
    for (int i = 1; i < IPT; ++i) a[i] += a[i - 1];
    const double cex = block_excl_offset<NT>(a[IPT - 1], red0);
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2)
            *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{a[i] + cex, a[i + 1] + cex}};
    }
    __syncthreads();
    if (act) {
#pragma unroll
        for (int i = IPT - 1; i >= 1; --i) a[i] = base[(int)(se[i] >> 16) - 1] - (a[i - 1] + cex);
        a[0] = base[(int)(se[0] >> 16) - 1] - cex;
    }
    __syncthreads();
}

template <int IPT>
__device__ __forceinline__ void attr_load_se(const AttrArgs &A, int jl, unsigned (&se)[IPT]) {
#pragma unroll
    for (int i = 0; i < IPT; i += 2) {
        const TreeU2 u = *reinterpret_cast<const TreeU2 *>(A.tr.pack + jl + i);
        se[i] = (unsigned)u.v[0]; se[i + 1] = (unsigned)u.v[1];
    }
}

// a chunk's caller-side node indices (-1: a padding position or a thread beyond the tree)
__device__ __forceinline__ void attr_load_nd(const AttrArgs &A, bool act, int jl, int (&nd)[kAttrChunk]) {
    if (A.nop) {
#pragma unroll
        for (int i = 0; i < kAttrChunk; i += 4) {
            const int4 u = *reinterpret_cast<const int4 *>(A.nop + jl + i);
            nd[i] = u.x; nd[i + 1] = u.y; nd[i + 2] = u.z; nd[i + 3] = u.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kAttrChunk; ++i) nd[i] = jl + i;
    }
#pragma unroll
    for (int i = 0; i < kAttrChunk; ++i) nd[i] = (act && nd[i] >= 0 && nd[i] < A.n_out) ? nd[i] : -1;
}

// a chunk's bytes of a per-position uint8 array, one 8-byte load (NULL: every byte 1)
__device__ __forceinline__ unsigned long long attr_load_bytes(const uint8_t *p, int jl) {
    return p ? *reinterpret_cast<const unsigned long long *>(p + jl) : 0x0101010101010101ull;
}

// w' = w flow, the drop scan's terms (net_scans.h's net_times_w, under the same contraction setting)
template <int IPT>
__device__ __forceinline__ void attr_times_w(const TreeArgs &tr, bool act, int jl, double (&a)[IPT]) {
#pragma unroll
    for (int c = 0; c < IPT; c += kAttrChunk) {
#pragma unroll
        for (int i = 0; i < kAttrChunk; i += 2) {
            const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + jl + c + i);
            a[c + i] = act ? a[c + i] * wv.v[0] : 0.0; a[c + i + 1] = act ? a[c + i + 1] * wv.v[1] : 0.0;
        }
        ATTR_FENCE();
    }
}

// The drop scan (net_scans.h's net_path_scan): a[i] = the terms of this thread's positions (0 beyond the tree) -> their sums over the
// positions' ancestors-or-self.  Every earlier read of the LDS buffer must be done; ends without a barrier behind its own
// last reads.
template <int NT, int IPT>
__device__ __forceinline__ void attr_path_scan(const TreeArgs &tr, bool act, int jl, double *lds, double (&a)[IPT]) {
    const int j0 = IPT * threadIdx.x;
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT, *red1 = red0 + NT / 64;
    double b[IPT];
    unsigned ec[IPT];                                               // eo | cle << 16
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{a[i], a[i + 1]}};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IPT; i += 2) {
        const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
        ec[i] = (unsigned)(u.v[0] >> 32); ec[i + 1] = (unsigned)(u.v[1] >> 32);
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) b[i] = act ? base[(int)(ec[i] & 0xFFFFu)] : 0.0;
#pragma unroll
    for (int i = 1; i < IPT; ++i) { a[i] += a[i - 1]; b[i] += b[i - 1]; }
    const double pex = block_excl_offset<NT>(a[IPT - 1], red1);     // (its barrier: every read of the terms is done)
    const double fex = block_excl_offset<NT>(b[IPT - 1], red0);
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2)
            *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{b[i] + fex, b[i + 1] + fex}};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IPT; ++i) a[i] = (a[i] + pex) - base[act ? (int)(ec[i] >> 16) - 1 : -1];
}

// The largest `tot` (all >= 0) over the threads before (UP) or behind this one in the workgroup: a selection.  One
// barrier; `red` (NT / 64 doubles) must not be rewritten before the caller's next barrier.
template <int NT, bool UP>
__device__ __forceinline__ double block_excl_max(double tot, double *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double other = UP ? __shfl_up(incl, o) : __shfl_down(incl, o);
        if (UP ? lane >= o : lane + o < 64) incl = fmax(incl, other);
    }
    if (lane == (UP ? 63 : 0)) red[wave] = incl;
    const double next = UP ? __shfl_up(incl, 1) : __shfl_down(incl, 1);
    double off = (UP ? lane >= 1 : lane < 63) ? next : 0.0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NT / 64; ++w)
        if (UP ? w < wave : w > wave) off = fmax(off, red[w]);
    return off;
}

// (value, index, position) triples in the arg-max's order: the larger value, then the lower index; index -1: none
__device__ __forceinline__ void attr_better(double &bv, int &bi, int &bp, double ov, int oi, int op) {
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; bp = op; }
}

// Everything below rounds each operation on its own (the contract's IEEE operations): no product is fused into a sum.
#pragma clang fp contract(off)

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void net_attr_kernel(AttrArgs A0) {
    extern __shared__ double attr_lds[];
    double *lds = attr_lds;
    AttrArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y, lane = tid & 63, wave = tid >> 6;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T, cell = ((int64_t)sc * T + t) * n;
        A.g += (int64_t)sc * A.m * T;
        if (A.ev) A.ev += (int64_t)sc * A.m * T;
        if (A.sens) A.sens += arr;
        if (A.contrib) A.contrib += arr;
        if (A.evc) A.evc += arr;
        if (A.drop) A.drop += arr;
        if (A.stage) A.stage += cell;
        if (A.stage_ev) A.stage_ev += cell;
        if (A.flags) A.flags += cell;
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT, *red1 = red0 + NT / 64;
    unsigned long long *kbuf = reinterpret_cast<unsigned long long *>(base);       // the deposits of wc, as bit patterns
    double *sred = lds + attr_lds_doubles<NT, IPT>();               // [kAttrSums][16]
    double *mred = sred + kAttrSums * 16;                           // [16]
    int *ired = reinterpret_cast<int *>(mred + 16);                 // [16]
    int *pred = ired + 16;                                          // [16]
    double *wdrop = mred + 16 + 8 + 8;                              // the watched position's drop (a fixed watch_pos)
    int *wnode = reinterpret_cast<int *>(wdrop + 1);                // its caller-side index
    int *cnt = wnode + 1;                                           // n_reach, n_big, n_can
    const double nan = __builtin_nan("");
    if (tid == 0) {
        lds[1] = 0.0;                                               // base[-1]
        *wdrop = 0.0; *wnode = -1; cnt[0] = cnt[1] = cnt[2] = 0;
    }

    double a[IPT];
    bool bad = false;
    {
        unsigned se[IPT];
        attr_load_se<IPT>(A, jl, se);
        attr_flow_scan<NT, IPT>(A, t, lds, se, a, bad);
    }
    ATTR_FENCE();
    // ---- drop = the path sums of w flow
    attr_times_w<IPT>(tr, act, jl, a);
    attr_path_scan<NT, IPT>(tr, act, jl, lds, a);
    // ---- the drops out; the candidate of this thread, or the fixed position's drop and index
    double bv = 0.0;
    int bi = -1, bp = -1;
#pragma unroll
    for (int c = 0; c < IPT; c += kAttrChunk) {
        int nd[kAttrChunk];
        attr_load_nd(A, act, jl + c, nd);
        unsigned long long mk = 0ull;
        if (A.limit) {
            mk = *reinterpret_cast<const unsigned long long *>(A.limit + jl + c);
        } else {
#pragma unroll
            for (int i = 0; i < kAttrChunk; i += 2) {
                const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + c + i);
                mk |= (unsigned long long)((u.v[0] & 0xFFFFull) != 0ull) << (8 * i);
                mk |= (unsigned long long)((u.v[1] & 0xFFFFull) != 0ull) << (8 * i + 8);
            }
        }
#pragma unroll
        for (int i = 0; i < kAttrChunk; ++i) {
            const double d = a[c + i];
            if (A.drop && nd[i] >= 0) A.drop[(int64_t)nd[i] * T + t] = d;
            if (A.watch_pos < 0) {
                if (((mk >> (8 * i)) & 0xFFull) != 0ull) attr_better(bv, bi, bp, d, nd[i], j0 + c + i);
            } else if (act && j0 + c + i == A.watch_pos) {
                *wdrop = d; *wnode = nd[i];
            }
        }
        ATTR_FENCE();
    }
    const bool badslot = __syncthreads_or(bad ? 1 : 0) != 0;        // (its barrier: every read of F is done)
    int jstar = A.watch_pos, wn;
    double dw;
    if (A.watch_pos < 0) {                                          // (uniform)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o), op = __shfl_xor(bp, o);
            attr_better(bv, bi, bp, ov, oi, op);
        }
        if (lane == 0) { mred[wave] = bv; ired[wave] = bi; pred[wave] = bp; }
        __syncthreads();
        bv = mred[0]; bi = ired[0]; bp = pred[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) attr_better(bv, bi, bp, mred[w], ired[w], pred[w]);
        jstar = bi >= 0 ? bp : -1; dw = bv; wn = bi;
    } else {
        dw = *wdrop; wn = *wnode;
    }
    const bool none = !badslot && jstar < 0;                        // no candidate: every output +0.0
    if (badslot || jstar >= n) jstar = -1;
    if (jstar < 0) dw = 0.0;
    const double over = dw - A.drop_max;
    const double excess = over > 0.0 ? over : 0.0;
    const double big = A.frac * dw;

    // ---- sens: the prefix max of the marked wc up to j*, the suffix max of the deposits behind it
    double s[IPT], u[IPT];
    {
        unsigned se[IPT];
        attr_load_se<IPT>(A, jl, se);
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeU2 *>(kbuf + j0 + i) = TreeU2{{0ull, 0ull}};
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(A.wc + jl + i);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int at = j0 + i + e, end = (int)(se[i + e] >> 16);
                const bool marked = act && jstar >= 0 && at <= jstar && jstar < end && wv.v[e] > 0.0;
                s[i + e] = marked ? wv.v[e] : 0.0;
                if (marked && end >= 1 && end <= n)
                    atomicMax(kbuf + (end - 1), (unsigned long long)__double_as_longlong(wv.v[e]));
            }
        }
#pragma unroll
        for (int i = 1; i < IPT; ++i) s[i] = fmax(s[i], s[i - 1]);
        const double pre = block_excl_max<NT, true>(s[IPT - 1], red0);     // (its barrier: every deposit is made)
#pragma unroll
        for (int i = 0; i < IPT; ++i) s[i] = fmax(s[i], pre);
#pragma unroll
        for (int i = 0; i < IPT; ++i) u[i] = act ? __longlong_as_double((long long)kbuf[j0 + i]) : 0.0;
#pragma unroll
        for (int i = IPT - 2; i >= 0; --i) u[i] = fmax(u[i], u[i + 1]);
        const double suf = block_excl_max<NT, false>(u[0], red1);
#pragma unroll
        for (int i = 0; i < IPT; ++i) s[i] = (j0 + i <= jstar) ? s[i] : fmax(u[i], suf);
    }
    ATTR_FENCE();

    // ---- the products, the counts, the stores; this thread's subtrees of the six sums
    double half[IPT / kAttrChunk][kAttrSums];
    int n_reach = 0, n_big = 0, n_can = 0;
#pragma unroll
    for (int c = 0; c < IPT; c += kAttrChunk) {
        int nd[kAttrChunk];
        attr_load_nd(A, act, jl + c, nd);
        const unsigned long long om = attr_load_bytes(A.out_mask, jl + c);
        const unsigned long long cl = A.cls ? attr_load_bytes(A.cls, jl + c) : ~0ull;
        double cv[kAttrChunk], ec[kAttrChunk];
        double l1[kAttrSums], l2[kAttrSums];                       // the pair tree's pending nodes: one per level
        unsigned long long fl = 0ull;
#pragma unroll
        for (int i = 0; i < kAttrChunk; i += 2) {
            const TreeU2 pk = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + c + i);
            double leaf[kAttrSums][2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int row = (int)(pk.v[e] & 0xFFFFull) - 1;
                const bool ok = act && row >= 0 && row < A.m;
                const double gv = A.g[(int64_t)(ok ? row : 0) * T + t];
                const double xv = A.ev ? A.ev[(int64_t)(ok ? row : 0) * T + t] : 0.0;
                const double inj = ok ? gv : 0.0, evv = (ok && A.ev) ? xv : 0.0;
                const double sn = (act && !none) ? s[c + i + e] : 0.0;
                s[c + i + e] = sn;
                const double pc = none ? 0.0 : sn * inj, pe = none ? 0.0 : sn * evv;
                cv[i + e] = pc; ec[i + e] = pe;
                leaf[0][e] = pc; leaf[1][e] = pe;
                const int k = (int)((cl >> (8 * (i + e))) & 0xFFull);
#pragma unroll
                for (int q = 0; q < 4; ++q) leaf[2 + q][e] = (act && k == q && q < A.C) ? pc : 0.0;
                const bool summ = nd[i + e] >= 0 && ((om >> (8 * (i + e))) & 0xFFull) != 0ull && !none;
                const bool reach = summ && !badslot && sn > 0.0;
                const bool isbig = reach && pc > big;
                const bool can = reach && excess > 0.0 && excess / sn <= evv;
                n_reach += reach ? 1 : 0; n_big += isbig ? 1 : 0; n_can += can ? 1 : 0;
                fl |= (unsigned long long)((summ ? kAttrSummarised : 0u) | (reach ? kAttrReach : 0u) | (isbig ? kAttrBig : 0u))
                      << (8 * (i + e));
            }
#pragma unroll
            for (int q = 0; q < kAttrSums; ++q) {
                const double pair = leaf[q][0] + leaf[q][1];
                if ((i & 2) == 0) { l1[q] = pair; continue; }
                const double quad = l1[q] + pair;
                if ((i & 4) == 0) l2[q] = quad;
                else half[c / kAttrChunk][q] = l2[q] + quad;
            }
        }
#pragma unroll
        for (int i = 0; i < kAttrChunk; ++i) {
            if (badslot) { s[c + i] = nan; cv[i] = nan; ec[i] = nan; }
            if (nd[i] < 0) continue;
            if (A.sens) A.sens[(int64_t)nd[i] * T + t] = s[c + i];
            if (A.contrib) A.contrib[(int64_t)nd[i] * T + t] = cv[i];
            if (A.evc) A.evc[(int64_t)nd[i] * T + t] = ec[i];
        }
        if (act) {
            if (A.stage) {
#pragma unroll
                for (int i = 0; i < kAttrChunk; i += 2)
                    *reinterpret_cast<TreeD2 *>(A.stage + j0 + c + i) = TreeD2{{cv[i], cv[i + 1]}};
            }
            if (A.stage_ev) {
#pragma unroll
                for (int i = 0; i < kAttrChunk; i += 2)
                    *reinterpret_cast<TreeD2 *>(A.stage_ev + j0 + c + i) = TreeD2{{ec[i], ec[i + 1]}};
            }
            if (A.flags) *reinterpret_cast<unsigned long long *>(A.flags + j0 + c) = fl;
        }
        ATTR_FENCE();
    }
    if (!A.slot && !A.slot_scr) return;                             // (uniform)
    double root[kAttrSums];
#pragma unroll
    for (int q = 0; q < kAttrSums; ++q) {
        if constexpr (IPT == kAttrChunk) root[q] = half[0][q];
        else root[q] = half[0][q] + half[IPT / kAttrChunk - 1][q];
    }
    // ---- the fixed tree above the threads: lanes by an xor butterfly, then the wavefronts' roots level by level
    const int P = A.P;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if (o < P) {                                                // (uniform)
#pragma unroll
            for (int q = 0; q < kAttrSums; ++q) root[q] += __shfl_xor(root[q], o);
        }
        n_reach += __shfl_xor(n_reach, o); n_big += __shfl_xor(n_big, o); n_can += __shfl_xor(n_can, o);
    }
    const int W = P > 64 ? P / 64 : 1;
    if (lane == 0) {
        if (wave < W) {
#pragma unroll
            for (int q = 0; q < kAttrSums; ++q) sred[q * 16 + wave] = root[q];
        }
        if (n_reach) atomicAdd(cnt + 0, n_reach);
        if (n_big) atomicAdd(cnt + 1, n_big);
        if (n_can) atomicAdd(cnt + 2, n_can);
    }
    __syncthreads();
    if (tid < kAttrSums) {
        double *r = sred + tid * 16;
        for (int w = W; w > 1; w >>= 1)
            for (int i = 0; i < w / 2; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    }
    __syncthreads();
    if (tid == 0) {
        revs_attr_slot_t r;
        r.drop_watch = badslot ? nan : dw;
        r.excess = badslot ? nan : excess;
        r.total = badslot ? nan : sred[0];
        r.ev_total = badslot ? nan : sred[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) r.class_total[q] = badslot ? nan : (q < A.C ? sred[(2 + q) * 16] : 0.0);
#pragma unroll
        for (int k = 0; k < 8; ++k) { r.top_value[k] = nan; r.top_index[k] = -1; }
        r.watch = jstar >= 0 ? wn : -1;
        r.n_reach = cnt[0]; r.n_big = cnt[1]; r.n_can = cnt[2];
        r.n_bad = badslot ? 1 : 0;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        if (A.slot) A.slot[(size_t)sc * T + t] = r;
        if (A.slot_scr) A.slot_scr[(size_t)sc * T + t] = r;
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged contributions over the nodes that reach the
// watched one, then the eight of largest contribution into the slot record
constexpr int kAttrSumNT = 256;
struct AttrSumArgs {
    const double *stage;          // [S][T][n]
    const uint8_t *flags;         // [S][T][n]
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T], or NULL
    revs_attr_slot_t *slot;       // [S][T], or NULL: its top_value / top_index
    int32_t T, n, n_out;
};

template <class F>
__device__ __forceinline__ void attr_for_each(const AttrSumArgs &A, const double *row, const uint8_t *frow, F f) {
    for (int jb = 0; jb < A.n; jb += kAttrSumNT) {
        const int j = jb + (int)threadIdx.x;
        double v = __builtin_nan("");
        int nd = -1;
        unsigned fl = 0u;
        if (j < A.n) {
            nd = A.nop ? A.nop[j] : j;
            nd = (nd >= 0 && nd < A.n_out) ? nd : -1;
            fl = nd >= 0 ? (unsigned)frow[j] : 0u;
            v = row[j];
        }
        f(v, nd, fl);
    }
}

__global__ __launch_bounds__(kAttrSumNT) void attr_summary_kernel(AttrSumArgs A) {
    __shared__ BoxSelect<kAttrSumNT> sh;
    __shared__ double mv[kAttrSumNT / 64];
    __shared__ int mi[kAttrSumNT / 64];
    constexpr int NT = kAttrSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const uint8_t *frow = A.flags + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf();
    const double nan = __builtin_nan("");
    // box_select64's walk: an element is part of the sample when it is summarised, reaches the watched node and is no NaN
    auto walk = [&](auto f) {
        attr_for_each(A, row, frow, [&](double v, int nd, unsigned fl) {
            f(box_key(v), (fl & (kAttrSummarised | kAttrReach)) == (kAttrSummarised | kAttrReach) && v == v, v, (int)fl, nd);
        });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram
    double s[4] = {0.0, 0.0, 0.0, 0.0};           // values, NaNs, large shares, summarised without reach
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int fl, int) {
        const bool summ = ((unsigned)fl & kAttrSummarised) != 0u;
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (summ && v != v) ? 1.0 : 0.0;
        s[2] += (ok && ((unsigned)fl & kAttrBig)) ? 1.0 : 0.0;
        s[3] += (summ && v == v && !((unsigned)fl & kAttrReach)) ? 1.0 : 0.0;
        if (ok) { x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v); }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 4, true>(s, sh.red);
    block_reduce_multi<NT, 2, false>(x, sh.red);
    const int kcnt = (int)s[0];
    revs_net_summary_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.worst_value = nan;
    r.count = kcnt; r.n_fliers = 0; r.n_violations = (int)s[2]; r.n_nan = (int)s[1];
    r.worst_index = -1;
    r.reserved[0] = (int)s[3]; r.reserved[1] = r.reserved[2] = 0;
    revs_net_summary_t *out = A.out ? A.out + (size_t)sc * A.T + t : nullptr;
    if (kcnt == 0) {                              // (uniform; the slot record's top entries stay unused)
        if (tid == 0 && out) *out = r;
        return;
    }
    if (out) {                                    // (uniform)
        // ---- the selection; in its neighbour walk the worst node: the lowest caller-side index with the largest contribution
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
    if (!A.slot) return;                          // (uniform)
    // ---- the top 8 by eight arg-max rounds, each over the nodes after the last pick in (value down, index up) order
    revs_attr_slot_t *rec = A.slot + (size_t)sc * A.T + t;
    double pv = __builtin_inf();
    int pi = -1;                                   // the last pick: everything is after (+inf, -1)
    for (int k = 0; k < 8; ++k) {
        double bv = 0.0;
        int bi = -1;
        walk([&](unsigned long long, bool ok, double v, int, int nd) {
            if (ok && (v < pv || (v == pv && nd > pi))) arg_better(bv, bi, v, nd);
        });
        wave_argmax(bv, bi);
        __syncthreads();                           // (every read of mv / mi and of the reductions' LDS is done)
        if (lane == 0) { mv[wave] = bv; mi[wave] = bi; }
        __syncthreads();
        bv = mv[0]; bi = mi[0];
        for (int w = 1; w < NT / 64; ++w) arg_better(bv, bi, mv[w], mi[w]);
        if (tid == 0 && bi >= 0) { rec->top_index[k] = bi; rec->top_value[k] = bv; }
        if (bi >= 0) { pv = bv; pi = bi; }
        else { pv = -__builtin_inf(); pi = 0x7FFFFFFF; }       // (uniform) nothing is left
    }
}

// ---- the day of one (scenario, node): its contributions over the slots with an excess, the largest one and its earliest
// slot, the slots in which it carried a large share
struct AttrDayArgs {
    const double *stage, *stage_ev;   // [S][T][n]; stage_ev NULL without node_ev
    const uint8_t *flags;             // [S][T][n]
    const revs_attr_slot_t *slot;     // [S][T]
    const int32_t *nop;
    revs_attr_day_t *out;             // [S][n_out]
    int32_t S, T, n, n_out;
};

__global__ void attr_day_kernel(AttrDayArgs A) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.S * A.n) return;
    const int sc = idx / A.n, j = idx - sc * A.n;
    const int nd = A.nop ? A.nop[j] : j;
    if (nd < 0 || nd >= A.n_out) return;
    revs_attr_day_t r;
    r.sum = 0.0; r.ev_sum = 0.0; r.peak = __builtin_nan(""); r.peak_slot = -1; r.n_big = 0;
    for (int t = 0; t < A.T; ++t) {
        const revs_attr_slot_t *s = A.slot + (size_t)sc * A.T + t;
        if (s->n_bad) continue;                   // (a bad slot is left out)
        const int64_t at = ((int64_t)sc * A.T + t) * A.n + j;
        const double v = A.stage[at];
        if (s->excess > 0.0) {
            r.sum = r.sum + v;
            if (A.stage_ev) r.ev_sum = r.ev_sum + A.stage_ev[at];
        }
        if (r.peak_slot < 0 || v > r.peak) { r.peak = v; r.peak_slot = t; }
        r.n_big += (A.flags[at] & kAttrBig) ? 1 : 0;
    }
    A.out[(int64_t)sc * A.n_out + nd] = r;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_attribution_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (S < 1 || S > REVS_STUDY_MAX_S || T < 1 || T > REVS_MAX_T || tree_n < 1 || tree_n > REVS_TREE_MAX) return 0;
    return (int64_t)S * T * tree_n * 17 + (int64_t)S * T * (int64_t)sizeof(revs_attr_slot_t);
}

extern "C" int revs_net_attribution(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const revs_headroom_aux_t *aux,
                                    const double *node_g, const double *node_ev, const uint8_t *limit_mask,
                                    const uint8_t *out_mask, const uint8_t *class_of_pos, int32_t C, const int32_t *node_of_pos,
                                    int32_t n_out, int32_t watch_pos, double drop_max, double frac, double *sens_out,
                                    double *contrib_out, double *ev_contrib_out, double *drop_out, revs_attr_slot_t *slot_out,
                                    revs_net_summary_t *summary_out, revs_attr_day_t *day_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_attr_slot_t) == 192 && sizeof(revs_attr_day_t) == 32, "");
    const char *who = "revs_net_attribution";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0 && m <= 0xFFFF, "%s: m=%d outside 1..65535", who, (int)m);
    REVS_REQUIRE(node_g, "%s: null pointer argument node_g", who);
    const TreeArgs tr = tree_args(tree);
    REVS_REQUIRE(tree_form_ok(tr), "%s: " REVS_TREE_FORM_MSG, who, REVS_TREE_FORM_ARGS(tr, REVS_TREE_MAX));
    REVS_REQUIRE(n_out > 0 && n_out <= tr.n, "%s: n_out=%d outside 1..tree nodes", who, (int)n_out);
    REVS_REQUIRE(aux && aux->parent_pos && aux->wc, "%s: null aux, aux->parent_pos or aux->wc", who);
    REVS_REQUIRE(aux->n_jump >= 0 && aux->n_jump <= REVS_HEADROOM_MAX_JUMP, "%s: aux->n_jump=%d outside 0..%d", who,
                 (int)aux->n_jump, REVS_HEADROOM_MAX_JUMP);
    REVS_REQUIRE(aux->n_jump == 0 || aux->jump, "%s: aux->jump is NULL with n_jump > 0", who);
    REVS_REQUIRE(watch_pos >= -1 && watch_pos < tr.n, "%s: watch_pos=%d outside -1..tree nodes - 1", who, (int)watch_pos);
    REVS_REQUIRE(drop_max - drop_max == 0.0, "%s: drop_max is not finite", who);
    REVS_REQUIRE(frac - frac == 0.0 && frac >= 0.0, "%s: frac must be finite and >= 0", who);
    REVS_REQUIRE(C >= 0 && C <= 4, "%s: C=%d outside 0..4", who, (int)C);
    REVS_REQUIRE(C == 0 || class_of_pos, "%s: class_of_pos is NULL with C > 0", who);
    REVS_REQUIRE(sens_out || contrib_out || ev_contrib_out || drop_out || slot_out || summary_out || day_out,
                 "%s: every output is NULL", who);
    REVS_REQUIRE(!ev_contrib_out || node_ev, "%s: ev_contrib_out needs node_ev", who);
    const bool staged = slot_out || summary_out || day_out;
    REVS_REQUIRE(!staged || scratch, "%s: slot_out / summary_out / day_out need scratch (revs_net_attribution_scratch bytes)", who);
    REVS_REQUIRE(!staged || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    const size_t cells = (size_t)S * T * tr.n;
    double *stage = staged ? (double *)scratch : nullptr;
    double *stage_ev = (staged && node_ev) ? stage + cells : nullptr;
    revs_attr_slot_t *slot_scr = staged ? (revs_attr_slot_t *)((double *)scratch + 2 * cells) : nullptr;
    uint8_t *flags = staged ? (uint8_t *)(slot_scr + (size_t)S * T) : nullptr;
    AttrArgs A;
    A.tr = tr;
    A.g = node_g; A.ev = node_ev; A.wc = aux->wc; A.limit = limit_mask; A.out_mask = out_mask;
    A.cls = C > 0 ? class_of_pos : nullptr; A.nop = node_of_pos;
    A.m = m; A.T = T; A.n_out = n_out; A.C = C; A.watch_pos = watch_pos; A.drop_max = drop_max; A.frac = frac;
    {
        int p2 = 1;
        while (p2 < tr.n) p2 <<= 1;
        const int ipt = tree_shape(tr.n).ipt;
        A.P = p2 > ipt ? p2 / ipt : 1;
    }
    A.sens = sens_out; A.contrib = contrib_out; A.evc = ev_contrib_out; A.drop = drop_out;
    A.slot = slot_out; A.slot_scr = day_out ? slot_scr : nullptr;
    A.stage = stage; A.stage_ev = day_out ? stage_ev : nullptr; A.flags = flags;
    const int rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        return launch_lds(net_attr_kernel<nt(), ipt()>, dim3(T, S), dim3(nt()), attr_lds_bytes(tr.n), (hipStream_t)stream, who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out || slot_out) {
        AttrSumArgs P;
        P.stage = stage; P.flags = flags; P.nop = node_of_pos; P.out = summary_out; P.slot = slot_out;
        P.T = T; P.n = tr.n; P.n_out = n_out;
        hipLaunchKernelGGL(attr_summary_kernel, dim3(T, S), dim3(kAttrSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        AttrDayArgs D;
        D.stage = stage; D.stage_ev = stage_ev; D.flags = flags; D.slot = slot_scr; D.nop = node_of_pos; D.out = day_out;
        D.S = S; D.T = T; D.n = tr.n; D.n_out = n_out;
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(attr_day_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, D);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
