// The headroom report (include/revs_admm_ops.h, "headroom report"): per node and slot, the
// largest extra constant power that node could draw before a limit node's voltage drop reaches drop_max or a rated
// line on its root path reaches its rating -- and which of the two, where.
//
//   revs_net_headroom   net_headroom_kernel<NT, IPT>, the four shapes of tree_shape(), on revs_net_study's T x S grid;
//                       then headroom_summary_kernel (one workgroup per (slot, scenario), box_select64 of boxplot.h over
//                       the staged values) and headroom_day_kernel (one thread per (scenario, position))
//
// One workgroup per (slot, scenario):
//   1. the flow and the drop scans of the network report (net_scans.h, with the gather's test for a non-finite
//      injection; the drop scan's last step a chunk at a time, as net_report_kernel takes it): the same bits;
//   2. up:   A[a] = min of the slacks drop_max - drop[j] over the limit nodes of a's subtree, as ordered 64-bit keys in
//            the scans' LDS buffer.  Round r sends every position's current minimum to its 2^r-th ancestor by an LDS
//            atomic minimum.  In place: what a position holds is at every moment a minimum over some of its own
//            subtree, so a value that arrives early is still one of the target's; after round r a position has heard
//            from every descendant within 2^(r + 1) - 1 levels.  One barrier per round.
//   3. val[a] = min(A[a] / wc[a], rating[a] - flow[a]) (a term that does not exist: +inf), its kind in a bit array;
//   4. down: q[j] = min of val over j's ancestors-or-self, by the same jumps: q[j] = min(q[j], q[2^r-th ancestor]),
//            every read of a round before every write (two barriers);
//   5. the limiter: q never grows down a path, so the ancestors with q[a] == q[j] are j's nearest ones and the topmost
//            of them is where the minimum first appears -- the shallowest that attains it.  Binary lifting over the same
//            jumps finds it from LDS reads alone; no limiter travels through the rounds.
// Minima of keys are exact: any order gives the bits of tests/headroom_ref.py.  The rounds number bit_length(depth), not
// depth: a chain of 2048 takes 11, the 121144 feeder (depth 52) 6.
//
// LDS: the scans' buffer (8 bytes per position, reused for A, then q), their wave totals, one kind bit per position:
// tree_lds_bytes(n) + n / 8, 133 KB at 16 384 positions -- every shape runs the same path; the caller's scratch holds only the staged headrooms
// that the summary and the day kernel read.
#include "common.h"
#include "boxplot.h"
#include "net_scans.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

struct HeadArgs {
    TreeArgs tr;
    const double *g;              // node sums double[S][m][T]
    const double *rating;         // per position, or NULL
    const double *wc;             // per position: the resistance (x 2) of the path from the substation
    const uint8_t *limit;         // per position, or NULL (every position with a row)
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    const int32_t *parent;        // per position: the parent's position, -1
    const uint16_t *jump;         // [n_jump][n]: the 2^(r + 1)-th ancestor's position, 0xFFFF
    int32_t n_jump;
    int32_t m, T, n_out;
    double drop_max;
    double *head;                 // [S][n_out][T], or NULL
    int32_t *lim;                 // [S][n_out][T], or NULL
    double *drop, *flow;          // [S][n_out][T], or NULL
    double *stage;                // [S][T][n] by position, or NULL
};

__host__ __device__ inline size_t head_lds_bytes(int n) {
    const TreeShape sh = tree_shape(n);
    return tree_lds_bytes(n) + (size_t)sh.nt * sh.ipt / 8;
}

// thr[i] = rating - flow where the line above the position is rated, else +inf
template <int IPT>
__device__ __forceinline__ void head_thermal(const HeadArgs &A, int jl, const double (&flow)[IPT], double (&thr)[IPT]) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) thr[i] = __builtin_inf();
    if (A.rating) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeD2 u = *reinterpret_cast<const TreeD2 *>(A.rating + jl + i);
            if (u.v[0] > 0.0) thr[i] = u.v[0] - flow[i];
            if (u.v[1] > 0.0) thr[i + 1] = u.v[1] - flow[i + 1];
        }
    }
}

// The positions of the 2^r-th ancestors of kNetChunk consecutive positions from jl on (-1: none; an entry that is no
// earlier position -- a table that is not a preorder forest's -- is none as well: nothing is indexed by it).
__device__ __forceinline__ void head_anc_chunk(const HeadArgs &A, int r, int jl, int (&p)[kNetChunk]) {
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 4) {
            const int4 u = *reinterpret_cast<const int4 *>(A.parent + jl + i);
            p[i] = u.x; p[i + 1] = u.y; p[i + 2] = u.z; p[i + 3] = u.w;
        }
    } else {
        const uint4 u = *reinterpret_cast<const uint4 *>(A.jump + (size_t)(r - 1) * A.tr.n + jl);
        p[0] = (int)(u.x & 0xFFFFu); p[1] = (int)(u.x >> 16); p[2] = (int)(u.y & 0xFFFFu); p[3] = (int)(u.y >> 16);
        p[4] = (int)(u.z & 0xFFFFu); p[5] = (int)(u.z >> 16); p[6] = (int)(u.w & 0xFFFFu); p[7] = (int)(u.w >> 16);
    }
#pragma unroll
    for (int i = 0; i < kNetChunk; ++i) p[i] = (p[i] >= 0 && p[i] < jl + i) ? p[i] : -1;
}
__device__ __forceinline__ int head_anc_one(const HeadArgs &A, int r, int j) {
    const int p = r == 0 ? A.parent[j] : (int)A.jump[(size_t)(r - 1) * A.tr.n + j];
    return (p >= 0 && p < j) ? p : -1;
}

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void net_headroom_kernel(HeadArgs A0) {
    extern __shared__ double head_lds[];
    double *lds = head_lds;
    HeadArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y;
    {
        const int64_t arr = (int64_t)sc * A.n_out * T;
        A.g += (int64_t)sc * A.m * T;
        if (A.head) A.head += arr;
        if (A.lim) A.lim += arr;
        if (A.drop) A.drop += arr;
        if (A.flow) A.flow += arr;
        if (A.stage) A.stage += ((int64_t)sc * T + t) * n;
    }
    const TreeArgs &tr = A.tr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    unsigned long long *kbuf = reinterpret_cast<unsigned long long *>(lds + 2);    // A, then q: ordered keys by position
    unsigned char *kindb = reinterpret_cast<unsigned char *>(lds + 2 + NT * IPT + 2 * (NT / 64));     // one bit per position
    const unsigned long long kInf = box_key(__builtin_inf());
    // the 1024 x 16 shape has 128 registers per thread: it does not carry the thermal room through the drop scans but
    // runs the flow scan again behind them (the same bits: its order is fixed), as net_report_kernel does for its keys
    constexpr bool kRescan = IPT > 8;
    if (tid == 0) lds[1] = 0.0;                                     // base[-1]

    double a[IPT], thr[IPT];
    bool bad = false;
    {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, &bad);     // (A's fields, not locals: net_scans.h)
        net_flow_scan<NT, IPT>(act, lds, se, a);
    }
    NET_CHUNK_FENCE();
    const bool nanslot = __syncthreads_or(bad ? 1 : 0) != 0;        // the slot as a whole: one flag for the workgroup
    if constexpr (!kRescan) head_thermal<IPT>(A, jl, a, thr);
    // ---- flow out; w' = w flow
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        if (A.flow) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.flow[(int64_t)nd[i] * T + t] = a[c + i];
        }
        net_times_w_chunk<IPT>(tr, act, jl, c, a);
        NET_CHUNK_FENCE();
    }

    // ---- the drop scan, its last step a chunk at a time into the slack's key where j is a limit node
    unsigned long long key[IPT];
    {
        unsigned ec[IPT];
        double pex;
        net_path_prefix<NT, IPT>(tr, act, jl, lds, a, ec, pex);
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            const unsigned long long mk = net_limit_bytes(tr, A.limit, jl + c);
            int nd[kNetChunk];
            if (A.drop) net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) {
                const double d = net_path_at(act, lds, a[c + i], pex, ec[c + i]);
                if (A.drop && nd[i] >= 0) A.drop[(int64_t)nd[i] * T + t] = d;
                const bool lim = act && ((mk >> (8 * i)) & 0xFFu) != 0ull;
                key[c + i] = lim ? box_key(A.drop_max - d) : kInf;
            }
            NET_CHUNK_FENCE();
        }
    }
    __syncthreads();                                                // (every read of F is done)

    if (nanslot) {                                                  // (uniform) nothing of this slot is a headroom
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            int nd[kNetChunk];
            net_load_nd(A.nop, A.n_out, act, jl + c, nd);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) {
                if (nd[i] < 0) continue;
                if (A.head) A.head[(int64_t)nd[i] * T + t] = nan;
                if (A.lim) A.lim[(int64_t)nd[i] * T + t] = -1;
            }
        }
        if (A.stage && act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeD2 *>(A.stage + j0 + i) = TreeD2{{nan, nan}};
        }
        return;
    }

    if constexpr (kRescan) {
        unsigned se[IPT];
        net_load_se<IPT>(tr, jl, se);
        net_gather<IPT>(A.g, A.m, A.T, t, act, se, a, nullptr);
        net_flow_scan<NT, IPT>(act, lds, se, a);
        head_thermal<IPT>(A, jl, a, thr);
    }

    // ---- up: A[a] = the smallest slack among the limit nodes of a's subtree
    const int rounds = A.n_jump + 1;                                // (a forest of roots alone: its one round finds no parent)
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeU2 *>(kbuf + j0 + i) = TreeU2{{key[i], key[i + 1]}};
    }
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        if (act) {
#pragma unroll
            for (int c = 0; c < IPT; c += kNetChunk) {
                int p[kNetChunk];
                head_anc_chunk(A, r, j0 + c, p);
#pragma unroll
                for (int i = 0; i < kNetChunk; ++i) {
                    const unsigned long long k = kbuf[j0 + c + i];
                    if (p[i] >= 0 && k != kInf) atomicMin(kbuf + p[i], k);
                }
            }
        }
        __syncthreads();
    }
    // ---- the two terms of every position, the smaller one's key and kind (the voltage term first on a tie)
    {
        unsigned kbits = 0u;
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) {
                const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(A.wc + j0 + i);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const double av = box_val(kbuf[j0 + i + e]);
                    const double volt = wv.v[e] > 0.0 ? av / wv.v[e] : __builtin_inf();
                    const bool thermal = !(volt <= thr[i + e]);
                    key[i + e] = box_key(thermal ? thr[i + e] : volt);
                    kbits |= (thermal ? 1u : 0u) << (i + e);
                }
            }
#pragma unroll
            for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeU2 *>(kbuf + j0 + i) = TreeU2{{key[i], key[i + 1]}};
#pragma unroll
            for (int i = 0; i < IPT; i += 8) kindb[(j0 + i) >> 3] = (unsigned char)(kbits >> i);
        }
    }
    __syncthreads();
    // ---- down: q[j] = the smallest term among j's ancestors-or-self
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        if (act) {
#pragma unroll
            for (int c = 0; c < IPT; c += kNetChunk) {
                int p[kNetChunk];
                head_anc_chunk(A, r, j0 + c, p);
#pragma unroll
                for (int i = 0; i < kNetChunk; ++i) {
                    const unsigned long long k = kbuf[p[i] >= 0 ? p[i] : j0 + c + i];
                    key[c + i] = k < key[c + i] ? k : key[c + i];
                }
            }
        }
        __syncthreads();                                            // (every read of the round is done)
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeU2 *>(kbuf + j0 + i) = TreeU2{{key[i], key[i + 1]}};
        }
        __syncthreads();
    }
    // ---- out: the clamp, and the limiter -- the topmost of the nearest ancestors that share q[j]
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        net_load_nd(A.nop, A.n_out, act, jl + c, nd);
        double x[kNetChunk];
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) {
            const double q = box_val(key[c + i]);
            x[i] = q > 0.0 ? q : 0.0;
            if (A.head && nd[i] >= 0) A.head[(int64_t)nd[i] * T + t] = x[i];
        }
        if (A.stage && act) {
#pragma unroll
            for (int i = 0; i < kNetChunk; i += 2) *reinterpret_cast<TreeD2 *>(A.stage + j0 + c + i) = TreeD2{{x[i], x[i + 1]}};
        }
        if (A.lim) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) {
                if (nd[i] < 0) continue;
                int word = -1;
                if (key[c + i] != kInf) {
                    int at = j0 + c + i;
#pragma unroll 1
                    for (int r = rounds - 1; r >= 0; --r) {
                        const int p = head_anc_one(A, r, at);
                        if (p >= 0 && kbuf[p] == key[c + i]) at = p;
                    }
                    const int node = A.nop ? A.nop[at] : at;
                    const int kind = (kindb[at >> 3] >> (at & 7)) & 1;
                    word = (node >= 0 && node < A.n_out) ? (node | kind << 30) : -1;
                }
                A.lim[(int64_t)nd[i] * T + t] = word;
            }
        }
    }
}

// ---- the summary of one (slot, scenario): the box-plot record of the staged headrooms over the positions with out_mask
constexpr int kHeadSumNT = 256;
struct HeadSumArgs {
    const double *stage;          // [S][T][n]
    const uint8_t *mask;          // out_mask per position, or NULL
    const int32_t *nop;
    revs_net_summary_t *out;      // [S][T]
    int32_t T, n, n_out;
    double need;
};

__global__ __launch_bounds__(kHeadSumNT) void headroom_summary_kernel(HeadSumArgs A) {
    __shared__ BoxSelect<kHeadSumNT> sh;
    constexpr int NT = kHeadSumNT;
    const int tid = threadIdx.x, t = (int)blockIdx.x, sc = (int)blockIdx.y;
    const double *row = A.stage + ((int64_t)sc * A.T + t) * A.n;
    const double ninf = -__builtin_inf(), inf = __builtin_inf();
    // box_select64's walk: an element is part of the sample when it is summarised and finite
    auto walk = [&](auto f) {
        net_for_each<NT>(row, A.n, A.nop, A.n_out, A.mask, [&](double v, int nd, int) { f(box_key(v), nd >= 0 && v < inf, v, 0, nd); });
    };
    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram
    double s[4] = {0.0, 0.0, 0.0, 0.0};           // values, NaNs, unlimited, short of `need`
    double x[2] = {ninf, ninf};                   // -min, max
    walk([&](unsigned long long k, bool ok, double v, int, int nd) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += (nd >= 0 && v != v) ? 1.0 : 0.0;
        s[2] += (nd >= 0 && v == inf) ? 1.0 : 0.0;
        if (ok) {
            s[3] += v < A.need ? 1.0 : 0.0;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v);
        }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 4, true>(s, sh.red);
    block_reduce_multi<NT, 2, false>(x, sh.red);
    const int kcnt = (int)s[0];
    revs_net_summary_t r;
    const double nan = __builtin_nan("");
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.worst_value = nan;
    r.count = kcnt; r.n_fliers = 0; r.n_violations = (int)s[3]; r.n_nan = (int)s[1];
    r.worst_index = -1;
    r.reserved[0] = (int)s[2]; r.reserved[1] = r.reserved[2] = 0;
    revs_net_summary_t *out = A.out + (size_t)sc * A.T + t;
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    // ---- the selection; in its neighbour walk the worst node: the lowest caller-side index with the smallest headroom
    double wi[1] = {ninf};
    const BoxFigures b = box_select64(sh, kcnt, walk, [&](unsigned long long, bool ok, double v, int, int nd) {
        if (ok && -v == x[0]) wi[0] = fmax(wi[0], -(double)nd);
    });
    block_reduce_multi<NT, 1, false>(wi, sh.red);
    if (tid == 0) {
        r.min = -x[0]; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo; r.whisker_hi = b.whi;
        r.n_fliers = b.n_fliers;
        r.worst_value = -x[0]; r.worst_index = (int)-wi[0];
        *out = r;
    }
}

// ---- the day of one (scenario, node): the smallest headroom, its earliest slot, the slots short of `need`
__global__ void headroom_day_kernel(const double *stage, const int32_t *nop, revs_headroom_day_t *out, int S, int T, int n,
                                    int n_out, double need) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * n) return;
    const int sc = idx / n, j = idx - sc * n;
    const int nd = nop ? nop[j] : j;
    if (nd < 0 || nd >= n_out) return;
    revs_headroom_day_t r;
    r.min = __builtin_nan(""); r.slot = -1; r.n_short = 0;
    for (int t = 0; t < T; ++t) {
        const double v = stage[((int64_t)sc * T + t) * n + j];
        if (v != v) continue;                     // (a NaN slot is left out)
        if (r.slot < 0 || v < r.min) { r.min = v; r.slot = t; }
        r.n_short += v < need ? 1 : 0;
    }
    out[(int64_t)sc * n_out + nd] = r;
}

}  // namespace revs

using namespace revs;

extern "C" int64_t revs_net_headroom_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (!net_scratch_sizes_ok(S, T, tree_n)) return 0;
    return (int64_t)S * T * tree_n * (int64_t)sizeof(double);
}

extern "C" int revs_net_headroom(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const revs_headroom_aux_t *aux,
                                 const double *node_g, const double *rating, const uint8_t *limit_mask,
                                 const uint8_t *out_mask, const int32_t *node_of_pos, int32_t n_out, double drop_max,
                                 double need, double *headroom_out, int32_t *limiter_out, double *drop_out, double *flow_out,
                                 revs_net_summary_t *summary_out, revs_headroom_day_t *day_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_headroom_day_t) == 16, "");
    const char *who = "revs_net_headroom";
    TreeArgs tr;
    int rc = net_tree_checks(who, S, m, T, tree, node_g, " node_g", n_out, &tr);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(aux && aux->parent_pos && aux->wc, "%s: null aux, aux->parent_pos or aux->wc", who);
    REVS_REQUIRE(aux->n_jump >= 0 && aux->n_jump <= REVS_HEADROOM_MAX_JUMP, "%s: aux->n_jump=%d outside 0..%d", who,
                 (int)aux->n_jump, REVS_HEADROOM_MAX_JUMP);
    REVS_REQUIRE(aux->n_jump == 0 || aux->jump, "%s: aux->jump is NULL with n_jump > 0", who);
    REVS_REQUIRE(drop_max - drop_max == 0.0, "%s: drop_max is not finite", who);
    REVS_REQUIRE(need - need == 0.0 && need >= 0.0, "%s: need must be finite and >= 0", who);
    REVS_REQUIRE(headroom_out || limiter_out || drop_out || flow_out || summary_out || day_out, "%s: every output is NULL", who);
    const bool staged = summary_out || day_out;
    rc = net_scratch_checks(who, staged, scratch, "summary_out / day_out need", "revs_net_headroom_scratch");
    if (rc != REVS_OK) return rc;
    HeadArgs A;
    A.tr = tr;
    A.g = node_g; A.rating = rating; A.wc = aux->wc; A.limit = limit_mask; A.nop = node_of_pos;
    A.parent = aux->parent_pos; A.jump = aux->jump; A.n_jump = aux->n_jump;
    A.m = m; A.T = T; A.n_out = n_out; A.drop_max = drop_max;
    A.head = headroom_out; A.lim = limiter_out; A.drop = drop_out; A.flow = flow_out;
    A.stage = staged ? (double *)scratch : nullptr;
    rc = for_tree_shape(tr.n, [&](auto nt, auto ipt) {
        return launch_lds(net_headroom_kernel<nt(), ipt()>, dim3(T, S), dim3(nt()), head_lds_bytes(tr.n), (hipStream_t)stream, who, A);
    });
    if (rc != REVS_OK) return rc;
    if (summary_out) {
        HeadSumArgs P;
        P.stage = (const double *)scratch; P.mask = out_mask; P.nop = node_of_pos; P.out = summary_out;
        P.T = T; P.n = tr.n; P.n_out = n_out; P.need = need;
        hipLaunchKernelGGL(headroom_summary_kernel, dim3(T, S), dim3(kHeadSumNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    if (day_out) {
        const int64_t total = (int64_t)S * tr.n;
        hipLaunchKernelGGL(headroom_day_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double *)scratch, node_of_pos, day_out, (int)S, (int)T, (int)tr.n, (int)n_out, need);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
