// The network report (include/revs_admm_ops.h, "network report"): what the feeder looks like under a home
// profile -- the power through every line, its loading, the voltage of every node, and per slot the box-plot
// numbers of loading and voltage -- from the tree form of tree_body.h, one workgroup per slot.
//
//   revs_net_node_sums   node_g[m][t] = sum over the homes of m of (double) load + (double) p, one thread per
//                        (node, slot), the homes in ascending index, one accumulator: a fixed order
//   revs_net_node_sums_many   the same sums for the S scenarios of an ensemble, float[n][S][T] -> double[S][m][T]
//   revs_net_report      net_report_kernel<NT, IPT>, the four shapes of tree_shape()
//
// The scans are tree_scan's (tree_body.h), restated here with the two intermediate values kept that tree_scan
// multiplies away or masks: C[end_j] - C[j], the load of j's subtree, IS the flow of the line above j, and
// Pre[j] - F[cle_j] IS the voltage drop at j, checked row or not.  tree_body.h is not touched: the sweep's and the
// operator's kernels compile from the same text as before.  net_scans.h holds the same scans as pieces (the headroom and
// loss reports'); this kernel keeps its own text: from the pieces it was 1 to 2% slower on the study's 36-scenario grid.
//
// The summary's order statistics are exact and need no sort.  Every value summarised is a non-negative double
// (|flow| / rating, a square root), so its bit pattern orders like the value; the k-th smallest key is built bit by
// bit from the top, one count of "keys below the trial" per bit, for the three quartile ranks of both quantities at
// once: 63 rounds of IPT x 6 compares per thread (the compare's lane mask, a population count: no cross-lane
// reduction) and ONE barrier each, on values that never leave the registers.  A bitonic sort of the same 16 384
// doubles is 55 barrier-separated stages per quantity with 128 KB of LDS traffic in each.
#include "common.h"
#include "boxplot.h"
#include "tree_body.h"

#include <math.h>

namespace revs {

__global__ void net_node_sums_kernel(int m, int Ts, const int64_t *node_ptr, const float *load, const float *p,
                                     double *out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * Ts) return;
    const int node = idx / Ts, t = idx - node * Ts;
    const int64_t i0 = node_ptr[node], i1 = node_ptr[node + 1];
    double acc = 0.0;
    if (load) {
#pragma unroll 4
        for (int64_t i = i0; i < i1; ++i) acc += (double)load[i * Ts + t] + (double)p[i * Ts + t];
    } else {
#pragma unroll 4
        for (int64_t i = i0; i < i1; ++i) acc += (double)p[i * Ts + t];
    }
    out[idx] = acc;
}

// The same sums on an ensemble's layout: load / p float[n][S][Ts] (a residence's S Ts floats contiguous), out
// double[S][m][Ts], the study's.  One thread per (node, column c = s Ts + t), the column fastest: the reads are those
// of net_node_sums_kernel over the (n, S Ts) view, the transposition is in the one store.  The same accumulator,
// order and widening as above: scenario s's slice carries the bits of that kernel on scenario s's rows alone.
__global__ void net_node_sums_many_kernel(int m, int S, int Ts, const int64_t *node_ptr, const float *load, const float *p,
                                          double *out) {
    const int cols = S * Ts;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * cols) return;
    const int node = idx / cols, c = idx - node * cols;
    const int s = c / Ts, t = c - s * Ts;
    const int64_t i0 = node_ptr[node], i1 = node_ptr[node + 1];
    double acc = 0.0;
    if (load) {
#pragma unroll 4
        for (int64_t i = i0; i < i1; ++i) acc += (double)load[i * cols + c] + (double)p[i * cols + c];
    } else {
#pragma unroll 4
        for (int64_t i = i0; i < i1; ++i) acc += (double)p[i * cols + c];
    }
    out[((int64_t)s * m + node) * Ts + t] = acc;
}

struct NetArgs {
    TreeArgs tr;
    const double *g;              // node sums double[m][T]
    const double *rating;         // per position, or NULL
    const uint8_t *mask;          // per position, or NULL
    const int32_t *nop;           // node_of_pos, or NULL (identity)
    int32_t m, T, n_out;
    double vset2, vmin, vmax;
    double *flow, *loading, *volt;
    revs_net_summary_t *sum;      // [2][T], or NULL
    // the study (revs_net_study): blockIdx.y is the scenario; g, the three arrays and sum are strided by it
    double band[REVS_STUDY_MAX_BANDS];           // thresholds of the band counts (-inf: unused)
    int32_t *bandc;               // [S][T][nband], or NULL
    unsigned long long *stage;    // keys for the pooled selection [2][T][S][tr.n], or NULL
    int32_t nband;
};

constexpr unsigned long long kNoKey = ~0ull;     // an entry left out of the summary (no trial key is above 2^63)
constexpr unsigned long long kNanKey = ~0ull - 1;    // staged only: a rated line / masked node whose value is a NaN

// doubles behind the scans' LDS: kBlockRed per wavefront for the reductions, two count buffers of 16 bytes per wavefront
__host__ __device__ inline size_t net_lds_bytes(int n) {
    const TreeShape sh = tree_shape(n);
    return tree_lds_bytes(n) + sizeof(double) * (size_t)(sh.nt / 64) * (kBlockRed + 4);
}

__device__ __forceinline__ double key_val(unsigned long long k) { return __longlong_as_double((long long)k); }   // kNoKey: a NaN

// flow_j = C[end_j] - C[j] at this thread's positions (a), C the inclusive prefix of the injections in preorder.
// se[i]: the low half of pack (src + 1 | end << 16).  Ends behind a barrier: every read of C is done.
template <int NT, int IPT>
__device__ __forceinline__ void net_flow_scan(const NetArgs &A, int t, double *lds, const unsigned (&se)[IPT], double (&a)[IPT]) {
    const int tid = threadIdx.x, j0 = IPT * tid;
    const bool act = j0 < A.tr.n;
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {          // (positions without a row fetch row 0: straight-line loads, masked behind them)
        const int s = (int)(se[i] & 0xFFFFu) - 1;
        const bool ok = act && s >= 0 && s < A.m;
        const double v = A.g[(int64_t)(ok ? s : 0) * A.T + t];
        a[i] = ok ? v : 0.0;
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

// A chunk's caller-side node indices (-1: a padding position or a thread beyond the tree), ratings and mask bits:
// one branch on the optional array, vector loads behind it.
constexpr int kNetChunk = 8;       // positions whose side data (index, rating, mask) are in flight at once: the 1024 x 16
                                   // shape takes its 16 in two halves, fenced for the scheduler, to stay inside 128 registers
#define NET_CHUNK_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int IPT>
__device__ __forceinline__ void net_load_nd(const NetArgs &A, bool act, int jl, int (&nd)[IPT]) {
    if (A.nop) {
#pragma unroll
        for (int i = 0; i < IPT; i += 4) {
            const int4 u = *reinterpret_cast<const int4 *>(A.nop + jl + i);
            nd[i] = u.x; nd[i + 1] = u.y; nd[i + 2] = u.z; nd[i + 3] = u.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < IPT; ++i) nd[i] = jl + i;
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) nd[i] = (act && nd[i] >= 0 && nd[i] < A.n_out) ? nd[i] : -1;
}
template <int IPT>
__device__ __forceinline__ void net_load_rating(const NetArgs &A, int jl, double (&r)[IPT]) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) r[i] = 0.0;
    if (A.rating) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeD2 u = *reinterpret_cast<const TreeD2 *>(A.rating + jl + i);
            r[i] = u.v[0]; r[i + 1] = u.v[1];
        }
    }
}

// The key a line's loading enters the summary by (kNoKey: unrated, a padding position or a NaN), and the loading.
__device__ __forceinline__ unsigned long long net_loading_key(double flow, double r, bool valid, double &ld) {
    ld = r > 0.0 ? fabs(flow) / r : __builtin_nan("");
    return (valid && ld == ld) ? (unsigned long long)__double_as_longlong(ld + 0.0) : kNoKey;
}

// A chunk's keys into the staging row (by preorder position: 64 contiguous bytes per thread and chunk).
__device__ __forceinline__ void net_stage_chunk(unsigned long long *dst, const unsigned long long (&k)[kNetChunk]) {
#pragma unroll
    for (int i = 0; i < kNetChunk; i += 2) *reinterpret_cast<TreeU2 *>(dst + i) = TreeU2{{k[i], k[i + 1]}};
}

template <int NT, int IPT>
__global__ __launch_bounds__(NT) void net_report_kernel(NetArgs A0) {
    extern __shared__ double net_lds[];
    double *lds = net_lds;
    NetArgs A = A0;
    const int tid = threadIdx.x, t = (int)blockIdx.x, T = A.T, n = A.tr.n, j0 = IPT * tid;
    const int sc = (int)blockIdx.y, S = (int)gridDim.y;            // the scenario (revs_net_report: the only one)
    {
        const int64_t arr = (int64_t)sc * A.n_out * T;
        A.g += (int64_t)sc * A.m * T;
        if (A.flow) A.flow += arr;
        if (A.loading) A.loading += arr;
        if (A.volt) A.volt += arr;
        if (A.sum) A.sum += (int64_t)sc * 2 * T;
    }
    const TreeArgs &tr = A.tr;
    // this (slot, scenario)'s staging rows: loading, volt
    unsigned long long *stl = A.stage ? A.stage + ((int64_t)t * S + sc) * n : nullptr;
    unsigned long long *stv = A.stage ? stl + (int64_t)T * S * n : nullptr;
    const bool act = j0 < n;
    const int jl = act ? j0 : 0;                                    // (threads beyond the tree load position 0's data, unused)
    double *base = lds + 2, *red0 = lds + 2 + NT * IPT, *red1 = red0 + NT / 64;
    double *red = red1 + NT / 64;                                   // block_reduce_multi's
    unsigned long long *cbuf = reinterpret_cast<unsigned long long *>(red + (NT / 64) * kBlockRed);   // [2][NT / 64][2]
    // Registers: the 1024 x 16 shape has 128 per thread, and IPT doubles are 2 IPT of them.  The packed indices are
    // held as the half a phase needs; and where IPT = 16 the loading keys are not carried through the voltage
    // scans beside a, b and those indices -- the flow scan is run again behind them (the same bits: its order is
    // fixed), two barriers against spills inside the selection's 63 rounds.
    constexpr bool kRescan = IPT > 8;
    if (tid == 0) lds[1] = 0.0;                                     // base[-1]

    double a[IPT], b[IPT];
    unsigned long long lkey[IPT], vkey[IPT];
    double nanl = 0.0, nanv = 0.0;                                  // rated lines / masked nodes whose value is a NaN
    {
        unsigned se[IPT];
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
            se[i] = (unsigned)u.v[0]; se[i + 1] = (unsigned)u.v[1];
        }
        net_flow_scan<NT, IPT>(A, t, lds, se, a);
    }
    // ---- flow and loading out; w' = w flow
#pragma unroll
    for (int c = 0; c < IPT; c += kNetChunk) {
        int nd[kNetChunk];
        double r[kNetChunk];
        unsigned long long sk[kNetChunk];
        net_load_nd<kNetChunk>(A, act, jl + c, nd);
        net_load_rating<kNetChunk>(A, jl + c, r);
        if (A.flow) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.flow[(int64_t)nd[i] * T + t] = a[c + i];
        }
#pragma unroll
        for (int i = 0; i < kNetChunk; ++i) {
            const bool rated = nd[i] >= 0 && r[i] > 0.0;
            const unsigned long long k = net_loading_key(a[c + i], r[i], rated, r[i]);      // (r: the loading from here)
            if constexpr (!kRescan) {
                lkey[c + i] = k;
                nanl += (rated && k == kNoKey) ? 1.0 : 0.0;
                sk[i] = (rated && k == kNoKey) ? kNanKey : k;
            }
        }
        if constexpr (!kRescan) {
            if (stl && act) net_stage_chunk(stl + j0 + c, sk);
        }
        if (A.loading) {
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i)
                if (nd[i] >= 0) A.loading[(int64_t)nd[i] * T + t] = r[i];
        }
#pragma unroll
        for (int i = 0; i < kNetChunk; i += 2) {
            const TreeD2 wv = *reinterpret_cast<const TreeD2 *>(tr.w + jl + c + i);
            a[c + i] = act ? a[c + i] * wv.v[0] : 0.0; a[c + i + 1] = act ? a[c + i + 1] * wv.v[1] : 0.0;
        }
        NET_CHUNK_FENCE();
    }
    if (act) {
#pragma unroll
        for (int i = 0; i < IPT; i += 2) *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{a[i], a[i + 1]}};
    }
    __syncthreads();

    // ---- the same values in end-order, both prefixes, drop_j = Pre[j] - F_excl[cle_j]
    {
        unsigned ec[IPT];                                           // eo | cle << 16
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
            ec[i] = (unsigned)(u.v[0] >> 32); ec[i + 1] = (unsigned)(u.v[1] >> 32);
        }
#pragma unroll
        for (int i = 0; i < IPT; ++i) b[i] = act ? base[(int)(ec[i] & 0xFFFFu)] : 0.0;
#pragma unroll
        for (int i = 1; i < IPT; ++i) { a[i] += a[i - 1]; b[i] += b[i - 1]; }
        const double pex = block_excl_offset<NT>(a[IPT - 1], red1); // (its barrier: every read of w' is done)
        const double fex = block_excl_offset<NT>(b[IPT - 1], red0);
        if (act) {
#pragma unroll
            for (int i = 0; i < IPT; i += 2)
                *reinterpret_cast<TreeD2 *>(base + j0 + i) = TreeD2{{b[i] + fex, b[i + 1] + fex}};
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            int nd[kNetChunk];
            unsigned long long sk[kNetChunk];
            net_load_nd<kNetChunk>(A, act, jl + c, nd);
            const unsigned long long mk = A.mask ? *reinterpret_cast<const unsigned long long *>(A.mask + jl + c) : ~0ull;
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) {
                const bool in = nd[i] >= 0 && ((mk >> (8 * i)) & 0xFFu) != 0ull;
                const double x = A.vset2 - ((a[c + i] + pex) - base[act ? (int)(ec[c + i] >> 16) - 1 : -1]);
                const double v = x < 0.0 ? __builtin_nan("") : sqrt(x);      // (collapse under LinDistFlow: a NaN, as numpy's)
                if (A.volt && nd[i] >= 0) A.volt[(int64_t)nd[i] * T + t] = v;
                vkey[c + i] = (in && v == v) ? (unsigned long long)__double_as_longlong(v + 0.0) : kNoKey;
                nanv += (in && v != v) ? 1.0 : 0.0;
                sk[i] = (in && v != v) ? kNanKey : vkey[c + i];
            }
            if (stv && act) net_stage_chunk(stv + j0 + c, sk);
            NET_CHUNK_FENCE();
        }
    }
    // ---- band counts: masked nodes with volt <= band[b] (an entry left out or a NaN is a NaN here: never counted)
    if (A.bandc) {
        double bc[REVS_STUDY_MAX_BANDS];
#pragma unroll
        for (int b = 0; b < REVS_STUDY_MAX_BANDS; ++b) bc[b] = 0.0;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const double v = key_val(vkey[i]);
#pragma unroll
            for (int b = 0; b < REVS_STUDY_MAX_BANDS; ++b) bc[b] += v <= A.band[b] ? 1.0 : 0.0;
        }
        block_reduce_multi<NT, REVS_STUDY_MAX_BANDS, true>(bc, red);
        if (tid == 0) {
            int32_t *o = A.bandc + ((int64_t)sc * T + t) * A.nband;
#pragma unroll
            for (int b = 0; b < REVS_STUDY_MAX_BANDS; ++b)
                if (b < A.nband) o[b] = (int)bc[b];
        }
    }
    if (!A.sum && !(kRescan && stl)) return;
    if constexpr (kRescan) {
        __syncthreads();                                            // (every read of F is done)
        unsigned se[IPT];
#pragma unroll
        for (int i = 0; i < IPT; i += 2) {
            const TreeU2 u = *reinterpret_cast<const TreeU2 *>(tr.pack + jl + i);
            se[i] = (unsigned)u.v[0]; se[i + 1] = (unsigned)u.v[1];
        }
        net_flow_scan<NT, IPT>(A, t, lds, se, a);
#pragma unroll
        for (int c = 0; c < IPT; c += kNetChunk) {
            int nd[kNetChunk];
            double r[kNetChunk];
            unsigned long long sk[kNetChunk];
            net_load_nd<kNetChunk>(A, act, jl + c, nd);
            net_load_rating<kNetChunk>(A, jl + c, r);
#pragma unroll
            for (int i = 0; i < kNetChunk; ++i) {
                const bool rated = nd[i] >= 0 && r[i] > 0.0;
                lkey[c + i] = net_loading_key(a[c + i], r[i], rated, r[i]);
                nanl += (rated && lkey[c + i] == kNoKey) ? 1.0 : 0.0;
                sk[i] = (rated && lkey[c + i] == kNoKey) ? kNanKey : lkey[c + i];
            }
            if (stl && act) net_stage_chunk(stl + j0 + c, sk);
            NET_CHUNK_FENCE();
        }
        if (!A.sum) return;
    }

    // ---- counts and extremes
    const double ninf = -__builtin_inf();
    double s[6] = {0.0, 0.0, nanl, nanv, 0.0, 0.0};                 // values, NaNs, violations of {loading, volt}
    double x[5] = {ninf, ninf, ninf, ninf, ninf};                   // -min L, max L, -min V, max V, largest excursion of V
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const double l = key_val(lkey[i]), v = key_val(vkey[i]);
        if (lkey[i] != kNoKey) {
            s[0] += 1.0; s[4] += l > 1.0 ? 1.0 : 0.0;
            x[0] = fmax(x[0], -l); x[1] = fmax(x[1], l);
        }
        if (vkey[i] != kNoKey) {
            s[1] += 1.0; s[5] += (v < A.vmin || v > A.vmax) ? 1.0 : 0.0;
            x[2] = fmax(x[2], -v); x[3] = fmax(x[3], v);
            x[4] = fmax(x[4], fmax(A.vmin - v, v - A.vmax));
        }
    }
    block_reduce_multi<NT, 6, true>(s, red);
    block_reduce_multi<NT, 5, false>(x, red);
    // the worst line / node: the lowest node index among those that attain the extreme
    double wi[2] = {ninf, ninf};
    double vworst = ninf;                                           // (a candidate's own voltage: the owner writes it below)
    int iworst = -1;
#pragma unroll
    for (int c = IPT - kNetChunk; c >= 0; c -= kNetChunk) {         // (descending: the thread's lowest index stays)
        int nd[kNetChunk];
        net_load_nd<kNetChunk>(A, act, jl + c, nd);
#pragma unroll
        for (int i = kNetChunk - 1; i >= 0; --i) {
            const double v = key_val(vkey[c + i]);                  // (a NaN for an entry left out: every test fails)
            if (key_val(lkey[c + i]) == x[1]) wi[0] = fmax(wi[0], -(double)nd[i]);
            if (fmax(A.vmin - v, v - A.vmax) == x[4] && -(double)nd[i] >= wi[1]) { wi[1] = -(double)nd[i]; iworst = nd[i]; vworst = v; }
        }
        NET_CHUNK_FENCE();
    }
    block_reduce_multi<NT, 2, false>(wi, red);

    // ---- the quartiles' lower order statistics: rank (k - 1) q / 4 of k values, q = 1, 2, 3, bit by bit
    const int kcnt[2] = {(int)s[0], (int)s[1]};
    int rank[6], rem[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const int r = (kcnt[e / 3] > 0 ? kcnt[e / 3] - 1 : 0) * (e % 3 + 1);
        rank[e] = r >> 2; rem[e] = r & 3;
    }
    unsigned long long ans[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    const int wave = tid >> 6;
#pragma unroll 1
    for (int bit = 62; bit >= 0; --bit) {
        unsigned long long trial[6];
        unsigned int c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 6; ++e) trial[e] = ans[e] | (1ull << bit);
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                c[e] += (unsigned)__popcll(__ballot(lkey[i] < trial[e]));
                c[3 + e] += (unsigned)__popcll(__ballot(vkey[i] < trial[3 + e]));
            }
        }
        // (a wavefront's counts are <= 64 IPT, the workgroup's <= 16 384: 16-bit fields never carry)
        unsigned long long *cb = cbuf + (size_t)(bit & 1) * (NT / 64) * 2;
        if ((tid & 63) == 0) {
            cb[2 * wave] = c[0] | (unsigned long long)c[1] << 16 | (unsigned long long)c[2] << 32;
            cb[2 * wave + 1] = c[3] | (unsigned long long)c[4] << 16 | (unsigned long long)c[5] << 32;
        }
        __syncthreads();        // (the one barrier of a round: the buffers alternate, and a wavefront that writes
                                //  round r + 2 has passed round r + 1's barrier, behind every read of round r)
        // the wavefronts' counts summed across the first NT / 64 lanes of a row (block_reduce_multi's way), by halves:
        // no field carries into the next
        unsigned d[4] = {0u, 0u, 0u, 0u};
        if ((tid & 63) < NT / 64) {
            const TreeU2 u = *reinterpret_cast<const TreeU2 *>(cb + 2 * (tid & 63));
            d[0] = (unsigned)u.v[0]; d[1] = (unsigned)(u.v[0] >> 32); d[2] = (unsigned)u.v[1]; d[3] = (unsigned)(u.v[1] >> 32);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] += (unsigned)dpp_i<0x128>((int)d[k]);
            d[k] += (unsigned)dpp_i<0x124>((int)d[k]);
            d[k] += (unsigned)dpp_i<0x122>((int)d[k]);
            d[k] += (unsigned)dpp_i<0x121>((int)d[k]);
            d[k] = __builtin_amdgcn_readfirstlane(d[k]);
        }
        const int tot[6] = {(int)(d[0] & 0xFFFFu), (int)(d[0] >> 16), (int)d[1], (int)(d[2] & 0xFFFFu), (int)(d[2] >> 16), (int)d[3]};
#pragma unroll
        for (int e = 0; e < 6; ++e)
            if (tot[e] <= rank[e]) ans[e] = trial[e];
    }

    // ---- their upper neighbours: the same value when it repeats past the rank, else the smallest value above it
    double cle[6], nxt[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) { cle[e] = 0.0; nxt[e] = ninf; }
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (lkey[i] != kNoKey) {
                if (lkey[i] <= ans[e]) cle[e] += 1.0; else nxt[e] = fmax(nxt[e], -key_val(lkey[i]));
            }
            if (vkey[i] != kNoKey) {
                if (vkey[i] <= ans[3 + e]) cle[3 + e] += 1.0; else nxt[3 + e] = fmax(nxt[3 + e], -key_val(vkey[i]));
            }
        }
    }
    block_reduce_multi<NT, 6, true>(cle, red);
    block_reduce_multi<NT, 6, false>(nxt, red);
    double qv[6];                                                   // Q1, median, Q3 of {loading, volt}
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double lo = key_val(ans[e]);
        const bool last = rank[e] + 1 >= kcnt[e / 3];               // (numpy clips the upper index to k - 1; the rule
                                                                    //  is boxplot.h's box_next_differs: keep them in step)
        const double hi = (last || (int)cle[e] > rank[e] + 1) ? lo : -nxt[e];
        qv[e] = box_quartile(lo, hi, (unsigned)rem[e]);
    }
    // ---- whiskers: the farthest datum within 1.5 IQR of the box (matplotlib.cbook.boxplot_stats), then the fliers
    double lim[4], wk[4] = {ninf, ninf, ninf, ninf};                // -whisker_lo, whisker_hi of {loading, volt}
#pragma unroll
    for (int q = 0; q < 2; ++q) box_limits(qv[3 * q], qv[3 * q + 2], lim[2 * q], lim[2 * q + 1]);
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const double l = key_val(lkey[i]), v = key_val(vkey[i]);    // (a NaN for an entry left out: every test fails)
        if (l >= lim[0]) wk[0] = fmax(wk[0], -l);
        if (l <= lim[1]) wk[1] = fmax(wk[1], l);
        if (v >= lim[2]) wk[2] = fmax(wk[2], -v);
        if (v <= lim[3]) wk[3] = fmax(wk[3], v);
    }
    block_reduce_multi<NT, 4, false>(wk, red);
    double wlo[2], whi[2], fl[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        wlo[q] = box_whisker_lo(qv[3 * q], wk[2 * q] != ninf, -wk[2 * q]);
        whi[q] = box_whisker_hi(qv[3 * q + 2], wk[2 * q + 1] != ninf, wk[2 * q + 1]);
    }
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const double l = key_val(lkey[i]), v = key_val(vkey[i]);
        fl[0] += box_is_flier(l, wlo[0], whi[0]) ? 1.0 : 0.0;
        fl[1] += box_is_flier(v, wlo[1], whi[1]) ? 1.0 : 0.0;
    }
    block_reduce_multi<NT, 2, true>(fl, red);

    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            revs_net_summary_t r;
            const bool any = kcnt[q] > 0;
            const double nan = __builtin_nan("");
            r.min = any ? -x[2 * q] : nan;
            r.q1 = any ? qv[3 * q] : nan;
            r.median = any ? qv[3 * q + 1] : nan;
            r.q3 = any ? qv[3 * q + 2] : nan;
            r.max = any ? x[2 * q + 1] : nan;
            r.whisker_lo = any ? wlo[q] : nan;
            r.whisker_hi = any ? whi[q] : nan;
            r.worst_value = nan;
            r.count = kcnt[q];
            r.n_fliers = any ? (int)fl[q] : 0;
            r.n_violations = (int)s[4 + q];
            r.n_nan = (int)s[2 + q];
            r.worst_index = any ? (int)-wi[q] : -1;
            r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
            if (any && q == 0) r.worst_value = x[1];
            A.sum[(size_t)q * T + t] = r;
        }
    }
    // the worst node's own voltage: its owner knows it (written behind thread 0's record)
    __syncthreads();
    if (kcnt[1] > 0 && iworst >= 0 && (double)iworst == -wi[1]) A.sum[(size_t)T + t].worst_value = vworst;
}


// ---- the pooled selection (revs_net_study, second launch): one workgroup per (slot, quantity, group) over the staged
// keys of the group's scenarios: pass 0 here, then box_select64 (boxplot.h).
constexpr int kPoolNT = 1024;
struct PoolArgs {
    const unsigned long long *stage;              // [2][T][S][n]
    const int32_t *nop;                           // node_of_pos, or NULL
    revs_net_pooled_t *out;                       // [G][2][T]
    int32_t S, T, n, n_out, g0, words;
    double vmin, vmax;
    unsigned long long member[kGroupMaskWords];   // [groups of this launch][words]: bit s of a group's mask: scenario s
};

// f(ordered key, ok, value, scenario, position) over every staged key of the group, every thread the same number of
// times (threads past the row's end see kNoKey): the callers' lane masks and reductions stay whole.  A staged value is
// a non-negative double, +0.0 for -0.0: its bits with the top bit set are its ordered key.  kNoKey and kNanKey come
// with that bit and lose it: not ok, a key below every ordered key of the sample -- no prefix of theirs is a prefix of
// an order statistic -- and a NaN for the value, which fails every test.  (All of this rests on the staged values
// being non-negative, as the parent's raw-bit keys did: a negative one would come with the top bit, too.)
template <class F>
__device__ __forceinline__ void pool_for_each(const PoolArgs &A, const unsigned long long *member, const unsigned long long *rows, F f) {
    for (int w = 0; w < A.words; ++w) {
        unsigned long long mk = member[w];
        while (mk) {
            const int s = 64 * w + (int)__builtin_ctzll(mk);
            mk &= mk - 1;
            const unsigned long long *row = rows + (int64_t)s * A.n;
            for (int jb = 0; jb < A.n; jb += 2 * kPoolNT) {
                const int j = jb + 2 * (int)threadIdx.x;
                TreeU2 k{{kNoKey, kNoKey}};
                if (j < A.n) k = *reinterpret_cast<const TreeU2 *>(row + j);       // (n is even: j + 1 < n)
                f(k.v[0] ^ 1ull << 63, (k.v[0] >> 63) == 0ull, key_val(k.v[0]), s, j);
                f(k.v[1] ^ 1ull << 63, (k.v[1] >> 63) == 0ull, key_val(k.v[1]), s, j + 1);
            }
        }
    }
}

__global__ __launch_bounds__(kPoolNT) void net_pool_kernel(PoolArgs A) {
    __shared__ BoxSelect<kPoolNT> sh;
    constexpr int NT = kPoolNT;
    const int tid = threadIdx.x;
    const int t = (int)blockIdx.x, q = (int)blockIdx.y, gl = (int)blockIdx.z;
    const unsigned long long *member = A.member + (size_t)gl * A.words;
    const unsigned long long *rows = A.stage + ((int64_t)q * A.T + t) * A.S * A.n;
    const double ninf = -__builtin_inf();
    const double vmin = A.vmin, vmax = A.vmax;
    // a value's excursion: the loading itself / the distance outside (negative: inside) the voltage band
    auto exc = [&](double v) { return q ? fmax(vmin - v, v - vmax) : v; };
    auto walk = [&](auto f) { pool_for_each(A, member, rows, f); };
    // (for the selection every element is "ok": the key and the value of one that is not keep it out by themselves,
    //  which spares the digit passes a second condition per count)
    auto walk_keys = [&](auto f) {
        pool_for_each(A, member, rows, [&](unsigned long long k, bool, double v, int s, int j) { f(k, true, v, s, j); });
    };

    for (int i = tid; i < 3 * 256; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    // ---- pass 0: counts and extremes, and the top digit's histogram (one prefix: the empty one)
    double s[3] = {0.0, 0.0, 0.0};                // values, NaNs, violations
    double x[3] = {ninf, ninf, ninf};             // -min, max, largest excursion
    walk([&](unsigned long long k, bool ok, double v, int, int) {
        s[0] += ok ? 1.0 : 0.0;
        s[1] += k == (kNanKey ^ 1ull << 63) ? 1.0 : 0.0;
        if (ok) {
            s[2] += (q ? (v < vmin || v > vmax) : v > 1.0) ? 1.0 : 0.0;
            x[0] = fmax(x[0], -v); x[1] = fmax(x[1], v); x[2] = fmax(x[2], exc(v));
        }
        hist_add(sh.hist, ok, (unsigned)(k >> 56));
    });
    block_reduce_multi<NT, 3, true>(s, sh.red);
    block_reduce_multi<NT, 3, false>(x, sh.red);
    const int kcnt = (int)s[0];
    revs_net_pooled_t r;
    const double nan = __builtin_nan("");
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.worst_value = nan;
    r.count = kcnt; r.n_fliers = 0; r.n_violations = (int)s[2]; r.n_nan = (int)s[1];
    r.worst_index = r.worst_scenario = -1;
    r.reserved[0] = r.reserved[1] = 0;
    revs_net_pooled_t *out = A.out + ((size_t)(A.g0 + gl) * 2 + q) * A.T + t;
    if (kcnt == 0) {                              // (uniform)
        if (tid == 0) *out = r;
        return;
    }
    // ---- the selection; in its neighbour walk the worst entry: the largest excursion, lowest scenario, then lowest index
    double wcode = ninf, vworst = nan;            // -(scenario * 65536 + caller's index): exact in a double
    const BoxFigures b = box_select64(sh, kcnt, walk_keys, [&](unsigned long long, bool, double v, int sidx, int j) {
        if (exc(v) == x[2]) {
            const int nd = A.nop ? A.nop[j] : j;
            const double code = -((double)sidx * 65536.0 + (double)nd);
            if (code > wcode) { wcode = code; vworst = v; }
        }
    });
    double wc[1] = {wcode};
    block_reduce_multi<NT, 1, false>(wc, sh.red);
    if (tid == 0) {
        const long long code = (long long)-wc[0];
        r.min = -x[0]; r.q1 = b.q[0]; r.median = b.q[1]; r.q3 = b.q[2]; r.max = x[1];
        r.whisker_lo = b.wlo; r.whisker_hi = b.whi;
        r.n_fliers = b.n_fliers;
        r.worst_scenario = (int)(code >> 16); r.worst_index = (int)(code & 0xFFFF);
        if (q == 0) r.worst_value = x[1];
        *out = r;
    }
    // the worst node's own voltage: its owner knows it (written behind thread 0's record)
    __syncthreads();
    if (q == 1 && wcode == wc[0]) out->worst_value = vworst;
}

}  // namespace revs

using namespace revs;

extern "C" int revs_net_node_sums(int32_t m, int32_t T, const int64_t *node_ptr, const float *load, const float *p,
                                  double *node_g, void *stream) {
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "revs_net_node_sums: T=%d outside 1..%d", (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0, "revs_net_node_sums: m > 0 required");
    REVS_REQUIRE(node_ptr && p && node_g, "revs_net_node_sums: null pointer argument");
    const int64_t total = (int64_t)m * T;
    hipLaunchKernelGGL(net_node_sums_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       m, T, node_ptr, load, p, node_g);
    REVS_CHECK_LAUNCH("revs_net_node_sums");
    return REVS_OK;
}

extern "C" int revs_net_node_sums_many(int32_t S, int32_t m, int32_t T, const int64_t *node_ptr, const float *load,
                                       const float *p, double *node_g, void *stream) {
    const char *who = "revs_net_node_sums_many";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0 && m <= 0xFFFF, "%s: m=%d outside 1..65535", who, (int)m);
    const int64_t total = (int64_t)m * S * T;
    REVS_REQUIRE(total < ((int64_t)1 << 31), "%s: m*S*T=%lld outputs, 2^31 or more", who, (long long)total);
    REVS_REQUIRE(node_ptr, "%s: null pointer argument node_ptr", who);
    REVS_REQUIRE(p, "%s: null pointer argument p", who);
    REVS_REQUIRE(node_g, "%s: null pointer argument node_g", who);
    hipLaunchKernelGGL(net_node_sums_many_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       m, S, T, node_ptr, load, p, node_g);
    REVS_CHECK_LAUNCH(who);
    return REVS_OK;
}

// revs_net_report's and revs_net_study's common checks, and their launch on a T x S grid
static int net_report_check(const char *who, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                            int32_t n_out, double vset, double vmin, double vmax) {
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(m > 0 && m <= 0xFFFF, "%s: m=%d outside 1..65535", who, (int)m);
    REVS_REQUIRE(node_g, "%s: null pointer argument", who);
    const TreeArgs tr = tree_args(tree);
    REVS_REQUIRE(tree_form_ok(tr), "%s: " REVS_TREE_FORM_MSG, who, REVS_TREE_FORM_ARGS(tr, REVS_TREE_MAX));
    REVS_REQUIRE(n_out > 0 && n_out <= tr.n, "%s: n_out=%d outside 1..tree nodes", who, (int)n_out);
    REVS_REQUIRE(vset == vset && vset >= 0.0 && vset < INFINITY, "%s: vset must be finite and >= 0", who);
    REVS_REQUIRE(vmin <= vmax, "%s: vmin > vmax", who);                 // (also rejects NaN)
    return REVS_OK;
}

static int net_report_launch(const char *who, int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                             const double *rating, const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out,
                             double vset, double vmin, double vmax, const double *band, int32_t B, double *flow_out,
                             double *loading_out, double *volt_out, revs_net_summary_t *summary_out,
                             int32_t *band_count_out, void *stage, void *stream) {
    NetArgs A;
    A.tr = tree_args(tree);
    A.g = node_g; A.rating = rating; A.mask = node_mask; A.nop = node_of_pos;
    A.m = m; A.T = T; A.n_out = n_out;
    A.vset2 = vset * vset; A.vmin = vmin; A.vmax = vmax;
    A.flow = flow_out; A.loading = loading_out; A.volt = volt_out; A.sum = summary_out;
    for (int b = 0; b < REVS_STUDY_MAX_BANDS; ++b) A.band[b] = b < B ? band[b] : -INFINITY;
    A.bandc = B > 0 ? band_count_out : nullptr; A.nband = B;
    A.stage = (unsigned long long *)stage;
    return for_tree_shape(tree->n, [&](auto nt, auto ipt) {
        return launch_lds(net_report_kernel<nt(), ipt()>, dim3(T, S), dim3(nt()), net_lds_bytes(tree->n), (hipStream_t)stream, who, A);
    });
}

extern "C" int revs_net_report(int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g, const double *rating,
                               const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out, double vset,
                               double vmin, double vmax, double *flow_out, double *loading_out, double *volt_out,
                               revs_net_summary_t *summary_out, void *stream) {
    const char *who = "revs_net_report";
    const int rc = net_report_check(who, m, T, tree, node_g, n_out, vset, vmin, vmax);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(flow_out || loading_out || volt_out || summary_out, "%s: every output is NULL", who);
    return net_report_launch(who, 1, m, T, tree, node_g, rating, node_mask, node_of_pos, n_out, vset, vmin, vmax, nullptr, 0,
                             flow_out, loading_out, volt_out, summary_out, nullptr, nullptr, stream);
}

extern "C" int64_t revs_net_study_scratch(int32_t S, int32_t T, int32_t tree_n) {
    if (S < 1 || S > REVS_STUDY_MAX_S || T < 1 || T > REVS_MAX_T || tree_n < 1 || tree_n > REVS_TREE_MAX) return 0;
    return (int64_t)2 * S * T * tree_n * (int64_t)sizeof(unsigned long long);
}

extern "C" int revs_net_study(int32_t S, int32_t m, int32_t T, const revs_tree_t *tree, const double *node_g,
                              const double *rating, const uint8_t *node_mask, const int32_t *node_of_pos, int32_t n_out,
                              double vset, double vmin, double vmax, const int32_t *group, int32_t G, const double *band,
                              int32_t B, double *flow_out, double *loading_out, double *volt_out,
                              revs_net_summary_t *summary_out, revs_net_pooled_t *pooled_out, int32_t *band_count_out,
                              void *scratch, void *stream) {
    static_assert(sizeof(revs_net_pooled_t) == 96 && sizeof(revs_net_pooled_t) == sizeof(revs_net_summary_t), "");
    const char *who = "revs_net_study";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    const int rc = net_report_check(who, m, T, tree, node_g, n_out, vset, vmin, vmax);
    if (rc != REVS_OK) return rc;
    REVS_REQUIRE(G >= 0 && G <= S, "%s: G=%d outside 0..S", who, (int)G);
    REVS_REQUIRE(B >= 0 && B <= REVS_STUDY_MAX_BANDS, "%s: B=%d outside 0..%d", who, (int)B, REVS_STUDY_MAX_BANDS);
    REVS_REQUIRE(G == 0 || group, "%s: group is NULL with G > 0", who);
    REVS_REQUIRE(B == 0 || band, "%s: band is NULL with B > 0", who);
    for (int s = 0; s < S && G > 0; ++s)
        REVS_REQUIRE(group[s] >= -1 && group[s] < G, "%s: group[%d]=%d outside -1..G-1", who, s, (int)group[s]);
    for (int b = 0; b < B; ++b)
        REVS_REQUIRE(band[b] - band[b] == 0.0, "%s: band[%d] is not finite", who, b);
    const bool bands = B > 0 && band_count_out, pooled = pooled_out != nullptr;
    REVS_REQUIRE(flow_out || loading_out || volt_out || summary_out || pooled || bands, "%s: every output is NULL", who);
    REVS_REQUIRE(!pooled || G > 0, "%s: pooled_out with G == 0", who);
    REVS_REQUIRE(!pooled || scratch, "%s: pooled_out needs scratch (revs_net_study_scratch bytes)", who);
    REVS_REQUIRE(!pooled || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    const int rc2 = net_report_launch(who, S, m, T, tree, node_g, rating, node_mask, node_of_pos, n_out, vset, vmin, vmax, band,
                                      bands ? B : 0, flow_out, loading_out, volt_out, summary_out, band_count_out,
                                      pooled ? scratch : nullptr, stream);
    if (rc2 != REVS_OK || !pooled) return rc2;
    PoolArgs P;
    P.stage = (const unsigned long long *)scratch; P.nop = node_of_pos; P.out = pooled_out;
    P.S = S; P.T = T; P.n = tree->n; P.n_out = n_out; P.words = (S + 63) / 64;
    P.vmin = vmin; P.vmax = vmax;
    for (int g0 = 0, ng; g0 < G; g0 += ng) {
        ng = pack_group_masks(group, S, G, g0, P.member);
        P.g0 = g0;
        hipLaunchKernelGGL(net_pool_kernel, dim3(T, 2, ng), dim3(kPoolNT), 0, (hipStream_t)stream, P);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
