// The two block scans over the feeder tree that every tree report opens with (DESIGN.md sections 3.7, 3.15, 3.16, 3.19
// 3.20, 3.21 and 3.22), and what goes with them, as pieces a report's kernel is put together from: headroom_kernels.hip's,
// losses_kernels.hip's, risk_kernels.hip's, price_kernels.hip's and powerflow_kernels.hip's (every pass of its loop) are.  A report whose flow and drop come from these pieces carries the bytes of revs_net_report.
// network_kernels.hip and attribution_kernels.hip hold the same scans in their own text: put together from these pieces
// net_report_kernel and net_attr_kernel were 1 to 2% slower on grids of 30 and more scenarios
// (profiles/net_scans_refactor_times.json).  A change to a scan is made in the three places.
//
//   the flow scan   net_gather, then net_flow_scan: flow[j] = C[end_j] - C[j], the subtree sums of the gathered node
//                   injections, C their inclusive prefix in preorder
//   the drop scan   net_times_w, then net_path_scan: drop[j] = Pre[j] - F_excl[cle_j], the path sums of w flow over the
//                   ancestors-or-self, Pre the prefix in preorder and F the prefix in end-order
//
// The scans are tree_scan's (tree_body.h: the solver's, on the hot path, not touched) with the two intermediate values
// kept that tree_scan multiplies away or masks.  A workgroup of NT threads owns IPT consecutive positions a thread; `lds`
// is the kernel's tree_lds_bytes() buffer, `act` whether the thread's positions lie inside the tree, jl its first
// position (0 for a thread beyond the tree: it loads position 0's data and uses none of it).
//
// net_path_scan is net_path_prefix and, per position, net_path_at.  net_headroom_kernel calls those two itself: its
// 1024 x 16 shape sits on 128 registers, and taking a chunk's drops straight into the chunk's consumer (the slack's key)
// keeps the 16 finished drops from being live beside the 16 prefixes.
// The last step is still this file's net_path_at, so nothing of the scan is restated there; the other kernels need no
// hook for it.
//
// Every piece takes TreeArgs and plain values and is inlined; nothing here asks which report calls it.  Each piece holds
// only additions or only multiplications, so the contraction setting at its definition cannot change a result: keep it
// that way (no product and sum in one piece).  No #pragma is set here, and the files include this header in front of
// their own `fp contract(off)`, where the copies it replaces stood: every kernel compiles the pieces alike.
#pragma once

#include "common.h"
#include "tree_body.h"

namespace revs {

constexpr int kNetChunk = 8;       // positions whose side data (index, rating, mask) are in flight at once: the 1024 x 16
                                   // shape takes its 16 in two halves, fenced for the scheduler, to stay inside 128 registers
#define NET_CHUNK_FENCE() __builtin_amdgcn_sched_barrier(0)

// doubles of a kernel's LDS in front of what it keeps behind the scans' buffer (tree_lds_doubles_even at compile time)
template <int NT, int IPT>
constexpr size_t net_lds_doubles() { return (2 + (size_t)NT * IPT + 2 * (NT / 64) + 1) / 2 * 2; }

// se[i]: the low half of pack (src + 1 | end << 16)
template <int IPT>
__device__ __forceinline__ void net_load_se(const TreeArgs &tr, int jl, unsigned (&se)[IPT]) {
#pragma unroll
    for (int i = 0; i < IPT; i += 2) {
        const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
        se[i] = (unsigned)u.v[0]; se[i + 1] = (unsigned)u.v[1];
    }
}

// a[i] = column t of the row of g (double[m][T]) that the position carries, 0 without one.  bad != NULL: *bad |= one of
// them is not finite.  g, m and T come by reference and a caller passes the FIELDS of its kernel's argument struct
// (A.g, A.m, A.T), not locals copied from them: they are then read where they are used and not held across the kernel.
// This steers this compiler's register allocation and nothing else, so a new caller that passes locals computes the
// same and loses only that; the figures to watch are profiles/net_scans_refactor_resources.json's.
template <int IPT>
__device__ __forceinline__ void net_gather(const double *const &g, const int32_t &m, const int32_t &T, int t, bool act,
                                           const unsigned (&se)[IPT], double (&a)[IPT], bool *bad) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {          // (positions without a row fetch row 0: straight-line loads, masked behind them)
        const int s = (int)(se[i] & 0xFFFFu) - 1;
        const bool ok = act && s >= 0 && s < m;
        const double v = g[(int64_t)(ok ? s : 0) * T + t];
        a[i] = ok ? v : 0.0;
        if (bad) *bad |= !(a[i] - a[i] == 0.0);
    }
}

// The gathered injections -> flow_j = C[end_j] - C[j] at this thread's positions.  Ends behind a barrier: every read of C
// is done.
template <int NT, int IPT>
__device__ __forceinline__ void net_flow_scan(bool act, double *lds, const unsigned (&se)[IPT], double (&a)[IPT]) {
    const int j0 = IPT * (int)threadIdx.x;
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT;
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

// A chunk's caller-side node indices (-1: a padding position or a thread beyond the tree): one branch on the optional
// array, vector loads behind it.
__device__ __forceinline__ void net_load_nd(const int32_t *nop, int n_out, bool act, int jl, int (&nd)[kNetChunk]) {
    if (nop) {
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 4) {
            const int4 u = *reinterpret_cast<const int4 *>(nop + jl + i);
            nd[i] = u.x; nd[i + 1] = u.y; nd[i + 2] = u.z; nd[i + 3] = u.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) nd[i] = jl + i;
    }
#pragma unroll
    for (int i = 0; i < kNetChunk; ++i) nd[i] = (act && nd[i] >= 0 && nd[i] < n_out) ? nd[i] : -1;
}

// a chunk's bytes of a per-position uint8 array, one 8-byte load (NULL: every byte 1)
__device__ __forceinline__ unsigned long long net_load_bytes(const uint8_t *p, int jl) {
    return p ? *reinterpret_cast<const unsigned long long *>(p + jl) : 0x0101010101010101ull;
}

// the chunk's limit nodes, a byte each: the mask's, or (no mask) whether the position carries a row
__device__ __forceinline__ unsigned long long net_limit_bytes(const TreeArgs &tr, const uint8_t *limit, int jl) {
    if (limit) return *reinterpret_cast<const unsigned long long *>(limit + jl);
    unsigned long long mk = 0ull;
#pragma unroll
    for (int i = 0; i < kNetChunk; i += 2) {
        const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
        mk |= (unsigned long long)((u.v[0] & 0xFFFFull) != 0ull) << (8 * i);
        mk |= (unsigned long long)((u.v[1] & 0xFFFFull) != 0ull) << (8 * i + 8);
    }
    return mk;
}

// w' = w flow, the drop scan's terms (0 beyond the tree): the chunk at c, and every chunk with its fence
template <int IPT>
__device__ __forceinline__ void net_times_w_chunk(const TreeArgs &tr, bool act, int jl, int c, double (&a)[IPT]) {
#pragma unroll
    for (int i = 0; i < kNetChunk; i += 2) {
        const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + jl + c + i);
        const double p0 = a[c + i] * wv.v[0], p1 = a[c + i + 1] * wv.v[1];     // (formed in every lane: the 16-byte load
        a[c + i] = act ? p0 : 0.0; a[c + i + 1] = act ? p1 : 0.0;              //  stays one load in front of a select)
    }
}
template <int IPT>
__device__ __forceinline__ void net_times_w(const TreeArgs &tr, bool act, int jl, double (&a)[IPT]) {
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        net_times_w_chunk<IPT>(tr, act, jl, c, a);
        NET_CHUNK_FENCE();
    }
}

// The drop scan up to its last step: a[i] = the terms of this thread's positions (0 beyond the tree) -> Pre[j] without
// the workgroup's offset pex; F, the prefix in end-order, in the LDS buffer; ec[i] = the high half of pack
// (eo | cle << 16).  Every earlier read of the LDS buffer must be done; ends behind a barrier: F is written.
template <int NT, int IPT>
__device__ __forceinline__ void net_path_prefix(const TreeArgs &tr, bool act, int jl, double *lds, double (&a)[IPT],
                                                unsigned (&ec)[IPT], double &pex) {
    const int j0 = IPT * (int)threadIdx.x;
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT, *red1 = red0 + NT / 64;
    double b[IPT];
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
    pex = block_excl_offset<NT>(a[IPT - 1], red1);                  // (its barrier: every read of the terms is done)
    const double fex = block_excl_offset<NT>(b[IPT - 1], red0);
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2)
            *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{b[i] + fex, b[i + 1] + fex}};
    }
    __syncthreads();
}
// ... and its last step at one position: the sum over the position's ancestors-or-self.
__device__ __forceinline__ double net_path_at(bool act, const double *lds, double a, double pex, unsigned ec) {
    return (a + pex) - (lds + 2)[act ? (int)(ec >> 16) - 1 : -1];
}

// The drop scan: a[i] = the terms -> their sums over the positions' ancestors-or-self.  Every earlier read of the LDS
// buffer must be done; ends without a barrier behind its own last reads.
template <int NT, int IPT>
__device__ __forceinline__ void net_path_scan(const TreeArgs &tr, bool act, int jl, double *lds, double (&a)[IPT]) {
    unsigned ec[IPT];
    double pex;
    net_path_prefix<NT, IPT>(tr, act, jl, lds, a, ec, pex);
#pragma unroll
    for (int i = 0; i < IPT; ++i) a[i] = net_path_at(act, lds, a[i], pex, ec[i]);
}

// The rows of a summary kernel (NT threads, one (slot, scenario) of staged values by position): f(value, caller-side
// index, position) over every position, every thread the same number of times -- threads past the row's end see a NaN
// and -1, as does a position without a caller-side index or (mask != NULL) outside the mask: the callers' lane masks and
// reductions stay whole.
template <int NT, class F>
__device__ __forceinline__ void net_for_each(const double *row, int n, const int32_t *nop, int n_out, const uint8_t *mask, F f) {
    for (int jb = 0; jb < n; jb += NT) {
        const int j = jb + (int)threadIdx.x;
        double v = __builtin_nan("");
        int nd = -1;
        if (j < n) {
            nd = nop ? nop[j] : j;
            nd = (nd >= 0 && nd < n_out && (!mask || mask[j] != 0)) ? nd : -1;
            v = row[j];
        }
        f(v, nd, j);
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------

// what the *_scratch functions answer 0 to
inline bool net_scratch_sizes_ok(int32_t S, int32_t T, int32_t tree_n) {
    return S >= 1 && S <= REVS_STUDY_MAX_S && T >= 1 && T <= REVS_MAX_T && tree_n >= 1 && tree_n <= REVS_TREE_MAX;
}

// The checks the reports' entry points share, in their order, and behind them the tree's arguments.  (g_name: " node_g";
// the network report's and the study's message ends before it.)  The checks of the staged outputs' scratch come behind
// the entry point's own ones: net_scratch_checks.
inline int net_tree_checks(const char *who, int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                           const char *g_name, int32_t n_out, TreeArgs *tr) {
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0 && m <= 0xFFFF, "%s: m=%d outside 1..65535", who, (int)m);
    REVS_REQUIRE(node_g, "%s: null pointer argument%s", who, g_name);
    *tr = tree_args(tree);
    REVS_REQUIRE(tree_form_ok(*tr), "%s: " REVS_TREE_FORM_MSG, who, REVS_TREE_FORM_ARGS(*tr, REVS_TREE_MAX));
    REVS_REQUIRE(n_out > 0 && n_out <= tr->n, "%s: n_out=%d outside 1..tree nodes", who, (int)n_out);
    return REVS_OK;
}
// `what` (the staged outputs, "summary_out / day_out") needs the scratch of `sizer` bytes, 16-byte aligned.
inline int net_scratch_checks(const char *who, bool staged, const void *scratch, const char *what, const char *sizer) {
    REVS_REQUIRE(!staged || scratch, "%s: %s scratch (%s bytes)", who, what, sizer);
    REVS_REQUIRE(!staged || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    return REVS_OK;
}

// threads that hold leaves of the fixed tree of a report's sums (fixed_tree.h): next_pow2(n) / IPT, at least 1
inline int32_t net_leaf_threads(int n) {
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    const int ipt = tree_shape(n).ipt;
    return p2 > ipt ? p2 / ipt : 1;
}

}  // namespace revs
