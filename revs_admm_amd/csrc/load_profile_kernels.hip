// The load-profile report (include/revs_admm_ops.h, "load-profile report"): per (scenario or
// group, class set, slot) the box-plot record of the residences' load, the same record over the residences' own daily
// peaks, and the day figures of the aggregate -- the demand curve of test-altered-profile.py:25-57, from a schedule
// where it lies on the device.
//
// A cell is (group, set, slot); a set is a class or, last, all classes together.  Unlike the convergence report's
// selection, where one workgroup owns a whole row of the history, the RESIDENCES are split over workgroups:
//
//   walk kernels   grid (residence chunks, slot tiles, scenarios), 1024 threads.  A workgroup reads the rows (i, s, :)
//                  of its chunk -- consecutive lanes on consecutive slots of a row, 16 bytes per lane where T % 4 == 0
//                  and the buffer allows it -- and keeps its tile's integers in LDS: class counters, 256-bin digit
//                  histograms per (slot, set, rank), keys of extremes / neighbours / whiskers.  LDS atomics once per
//                  distinct address of a wavefront (conv_add); at the end every non-zero word is merged into the
//                  cell's global word with one integer atomic (add / max).  No order to depend on.
//   pick kernels   one wavefront per cell between two walks: the bin that holds each open rank (prefix sum over the
//                  256 bins), the quartiles, the whisker limits.  Pass 0 takes the set "all" as the sum of the classes'
//                  counters and histograms; from the second digit on it has prefixes of its own, hence histograms.
//   total          the one floating sum: in the pass-0 walk every thread owns fixed slots and adds its rows in ascending
//                  order per class, the threads' sums meet in a fixed tree, the chunk's partial goes to scratch, and the
//                  finish kernel folds the chunks in a fixed order (64 interleaved runs, then the wavefront's butterfly).
//
// The sequence of a selection: pass 0, pick, [digit walk, pick] x 3, neighbour walk, quartiles, whisker walk, whiskers,
// flier walk, finish -- run for the slots per scenario, for the daily peaks per scenario (T = 1 over one float per
// (i, s) a row kernel leaves in scratch), and for both per group through a scenario -> group table.  A digit walk whose
// tile has no open rank, and a flier walk whose tile has no flier, return at once.
#include "common.h"
#include "boxplot.h"

#include <math.h>

// Every product and sum of this file is rounded on its own, as numpy's: no contraction to fused multiply-adds.
#pragma clang fp contract(off)

namespace revs {

constexpr int kProfNT = 1024;                     // threads of a walk workgroup
constexpr int kProfChunk = 512;                   // residences of a walk workgroup
constexpr int kProfHists = 144;                   // 1 KB histograms a digit walk keeps in LDS (of 160 KB per CU)
enum { kPcBad = 0, kPcNeg = 1, kPcZero = 2, kPcPos = 3, kPcAbove = 4, kPcN = 5 };

// A cell's state between the launches; all zeros at the start (one memset): keys that are minimised are held inverted.
struct ProfState {
    unsigned cnt[kPcN];                           // class sets: merged by pass 0; "all": summed by the pick
    unsigned ext_lo_inv, ext_hi;                  // ~key of the minimum, key of the maximum
    unsigned count, rank[3], rem4[3], left[3], eq[3], ans[3], open[3], need[3];
    unsigned nb_inv[3];                           // ~(the smallest key above ans)
    unsigned wk_lo_inv, wk_hi;                    // whisker candidates
    unsigned fl, any_fl;
    unsigned worst;                               // 2^31 - 1 - caller-side index of the largest value, maximised
    unsigned pad;
    double q[3], lim[2], w[2];
};

struct ProfArgs {
    const float *g;
    const uint8_t *cls;                           // [S][n] or NULL
    const int32_t *index;                         // [n] or NULL
    const int32_t *group_of;                      // [S] (-1: in no group) or NULL: scenario s is cell group s
    ProfState *st;                                // [NG][Q][T]
    unsigned *h0;                                 // [NG][ncls][T][256]: pass 0's histograms, per class
    unsigned *hg;                                 // [NG][Q][T][3][256]: the digit passes' histograms, per set and rank
    double *part;                                 // [chunks][S][ncls][T] or NULL (pools)
    const revs_bill_summary_t *member;            // pools: the scenarios' records [S][Q][T]
    revs_bill_summary_t *out;                     // [NG][Q][T]
    int64_t n, stride_s, stride_i;
    double above;
    int32_t S, T, ncls, Q, NG, TT, nchunks, pass;
};

__device__ __forceinline__ int prof_group(const ProfArgs &A, int s) { return A.group_of ? A.group_of[s] : s; }

// The rows of residences i0 .. i1 - 1 of scenario s, slots t0 .. t0 + tw - 1: thread (rl, col) of the first R tpr takes
// row ib + rl, slots t0 + V col .. + V - 1.  f(j, key, value, kind, class, tt, i) for every element of every thread
// (kind -1: none; kPcBad: not finite; else kPcNeg / kPcZero / kPcPos), the same number of calls in every thread.
template <int V, class F>
__device__ __forceinline__ void prof_walk(const ProfArgs &A, int s, int t0, int tw, int64_t i0, int64_t i1, F f) {
    const int tid = threadIdx.x, tpr = tw / V, R = kProfNT / tpr, rl = tid / tpr, col = tid - rl * tpr;
    const float *base = A.g + (int64_t)s * A.stride_s + t0 + V * col;
    for (int64_t ib = i0; ib < i1; ib += R) {
        const int64_t i = ib + rl;
        int c = -1;
        unsigned u[V];
#pragma unroll
        for (int j = 0; j < V; ++j) u[j] = 0u;
        if (rl < R && i < i1) {
            c = A.cls ? (int)A.cls[(int64_t)s * A.n + i] : 0;
            if (c >= A.ncls) c = -1;
            if (c >= 0) {
                const float *p = base + i * A.stride_i;
                if constexpr (V == 4) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(p);
                    u[0] = q.x; u[1] = q.y; u[2] = q.z; u[3] = q.w;
                } else {
                    u[0] = __float_as_uint(*p);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int kind = -1;
            unsigned key = 0u;
            double v = 0.0;
            if (c >= 0) {
                if ((u[j] & 0x7F800000u) == 0x7F800000u) kind = kPcBad;
                else {
                    key = box_key_f(u[j]);
                    v = box_val_f(key);
                    kind = key < kBoxKey0F ? kPcNeg : key == kBoxKey0F ? kPcZero : kPcPos;
                }
            }
            f(j, key, v, kind, c, V * col + j, i);
        }
    }
}

// what a walk workgroup works on; false: nothing (a scenario in no group)
struct ProfTile { int s, grp, t0, tw; int64_t i0, i1; };
__device__ __forceinline__ bool prof_tile(const ProfArgs &A, ProfTile &P) {
    P.s = blockIdx.z; P.grp = prof_group(A, P.s);
    P.t0 = blockIdx.y * A.TT; P.tw = min(A.TT, A.T - P.t0);
    P.i0 = (int64_t)blockIdx.x * kProfChunk; P.i1 = min(P.i0 + kProfChunk, A.n);
    return P.grp >= 0;
}
// the cell of set q, tile slot tt
__device__ __forceinline__ int64_t prof_cell(const ProfArgs &A, const ProfTile &P, int q, int tt) {
    return ((int64_t)P.grp * A.Q + q) * A.T + P.t0 + tt;
}

extern __shared__ __align__(16) unsigned prof_lds[];

// ---- pass 0: counts, extremes, the top digit's histogram per class, the chunk's partial totals
template <int V>
__global__ __launch_bounds__(kProfNT) void prof_pass0_kernel(ProfArgs A) {
    ProfTile P;
    if (!prof_tile(A, P)) return;
    const int tid = threadIdx.x, nc = A.ncls, ncell = P.tw * nc;
    unsigned *hist = prof_lds;                    // [tw][nc][256]
    unsigned *cnt = hist + ncell * 256;           // [tw][nc][8]
    unsigned *ext = cnt + ncell * 8;              // [tw][nc][2]: ~min, max
    for (int i = tid; i < ncell * (256 + 8 + 2); i += kProfNT) prof_lds[i] = 0u;
    __syncthreads();
    double acc[V][REVS_PROFILE_MAX_CLASSES];
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int c = 0; c < REVS_PROFILE_MAX_CLASSES; ++c) acc[j][c] = 0.0;
    prof_walk<V>(A, P.s, P.t0, P.tw, P.i0, P.i1, [&](int j, unsigned key, double v, int kind, int c, int tt, int64_t) {
        const unsigned lc = (unsigned)(tt * nc + (c < 0 ? 0 : c));
        const bool ok = kind > kPcBad;
        conv_add(cnt, kind >= 0, lc * 8 + (unsigned)(kind < 0 ? 0 : kind));
        conv_add(cnt, ok && v > A.above, lc * 8 + kPcAbove);
        conv_add(hist, ok, lc * 256 + (key >> 24));
        if (ok) {
            if (~key > ext[lc * 2]) atomicMax(&ext[lc * 2], ~key);
            if (key > ext[lc * 2 + 1]) atomicMax(&ext[lc * 2 + 1], key);
            if (A.part) {
#pragma unroll
                for (int cc = 0; cc < REVS_PROFILE_MAX_CLASSES; ++cc)
                    if (cc == c) acc[j][cc] = acc[j][cc] + v;
            }
        }
    });
    __syncthreads();
    // merge: every non-zero word into its cell's, with one integer atomic
    for (int i = tid; i < ncell * 256; i += kProfNT) {
        const unsigned v = hist[i];
        if (v) {
            const int lc = i >> 8, tt = lc / nc, c = lc - tt * nc;
            atomicAdd(A.h0 + ((((int64_t)P.grp * nc + c) * A.T + P.t0 + tt) << 8) + (i & 255), v);
        }
    }
    for (int i = tid; i < ncell * 8; i += kProfNT) {
        const unsigned v = cnt[i];
        const int lc = i >> 3, k = i & 7, tt = lc / nc, c = lc - tt * nc;
        if (v && k < kPcN) atomicAdd(&A.st[prof_cell(A, P, c, tt)].cnt[k], v);
    }
    for (int i = tid; i < ncell * 2; i += kProfNT) {
        const unsigned v = ext[i];
        const int lc = i >> 1, tt = lc / nc, c = lc - tt * nc;
        ProfState &st = A.st[prof_cell(A, P, c, tt)];
        if (v) atomicMax((i & 1) ? &st.ext_hi : &st.ext_lo_inv, v);
    }
    if (!A.part) return;                          // (uniform)
    // the chunk's partial totals: the threads of a column meet in a fixed tree, all (slot, class) pairs side by side
    __syncthreads();
    double *pt = reinterpret_cast<double *>(prof_lds);            // [V][nc][kProfNT]
    const int tpr = P.tw / V, R = kProfNT / tpr, rl = tid / tpr, col = tid - rl * tpr;
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int c = 0; c < REVS_PROFILE_MAX_CLASSES; ++c)
            if (c < nc) pt[(j * nc + c) * kProfNT + tid] = acc[j][c];
    __syncthreads();
    for (int h = kProfNT / 2; h >= 1; h >>= 1) {
        if (rl < h && rl + h < R) {
            for (int k = 0; k < V * nc; ++k)
                pt[k * kProfNT + tid] = pt[k * kProfNT + tid] + pt[k * kProfNT + tid + h * tpr];
        }
        __syncthreads();
    }
    if (rl == 0) {
        for (int j = 0; j < V; ++j)
            for (int c = 0; c < nc; ++c)
                A.part[(((int64_t)blockIdx.x * A.S + P.s) * nc + c) * A.T + P.t0 + V * col + j] = pt[(j * nc + c) * kProfNT + tid];
    }
}

// ---- the pick after pass 0 (A.pass == 0) or after the digit walk of pass 1..3: one wavefront per cell; every lane
// holds the cell's numbers, lane 0 writes them
__global__ __launch_bounds__(64) void prof_pick_kernel(ProfArgs A) {
    const int64_t cell = blockIdx.x;
    const int lane = threadIdx.x, t = (int)(cell % A.T), q = (int)((cell / A.T) % A.Q);
    const int64_t grp = cell / ((int64_t)A.T * A.Q);
    ProfState &st = A.st[cell];
    if (A.pass == 0) {
        const bool all = q >= A.ncls;             // the set of every class: the sum of the classes
        uint4 cc = make_uint4(0u, 0u, 0u, 0u);
        unsigned c5[kPcN] = {0u, 0u, 0u, 0u, 0u}, lo = 0u, hi = 0u;
        for (int c = all ? 0 : q; c < (all ? A.ncls : q + 1); ++c) {
            const uint4 x = *reinterpret_cast<const uint4 *>(A.h0 + (((grp * A.ncls + c) * A.T + t) << 8) + 4 * lane);
            cc.x += x.x; cc.y += x.y; cc.z += x.z; cc.w += x.w;
            const ProfState &sc = A.st[(grp * A.Q + c) * A.T + t];
            for (int k = 0; k < kPcN; ++k) c5[k] += sc.cnt[k];
            lo = max(lo, sc.ext_lo_inv); hi = max(hi, sc.ext_hi);
        }
        const unsigned nneg = c5[kPcNeg], nzero = c5[kPcZero], cnt = nneg + nzero + c5[kPcPos];
        if (lane == 0) {
            if (all) {                            // (the classes' cells keep these words as pass 0 left them)
                for (int k = 0; k < kPcN; ++k) st.cnt[k] = c5[k];
                st.ext_lo_inv = lo; st.ext_hi = hi;
            }
            st.count = cnt;
        }
        for (int e = 0; e < 3; ++e) {
            unsigned r, rem4;
            box_rank(cnt, e + 1, r, rem4);
            unsigned ans = 0u, left = r, eq = 0u;
            const unsigned open = (cnt && !box_settled_at_zero(r, nneg, nzero, ans, left, eq)) ? 1u : 0u;
            if (open) {                           // (uniform)
                unsigned bin;
                pick_bin(cc, r, bin, left, eq);
                ans = bin << 24;
            }
            if (lane == 0) {
                st.rank[e] = r; st.rem4[e] = rem4;
                st.ans[e] = ans; st.left[e] = left; st.eq[e] = eq; st.open[e] = open;
            }
        }
        return;
    }
    const int shift = 24 - 8 * A.pass;
    for (int e = 0; e < 3; ++e) {
        unsigned left = st.left[e], eq = st.eq[e];
        if (st.open[e]) {                         // (uniform)
            uint4 *h = reinterpret_cast<uint4 *>(A.hg + ((cell * 3 + e) << 8)) + lane;
            const uint4 cc = *h;
            *h = make_uint4(0u, 0u, 0u, 0u);      // (the next digit walk adds into zeros)
            unsigned bin;
            pick_bin(cc, left, bin, left, eq);
            if (lane == 0) { st.ans[e] |= bin << shift; st.left[e] = left; st.eq[e] = eq; }
        }
        if (A.pass == 3 && lane == 0) {
            // the upper neighbour: where the next order statistic is another value
            const unsigned cnt = st.count, r = st.rank[e], cle = r - left + eq;      // cle: values <= the statistic
            st.need[e] = (st.rem4[e] != 0u && box_next_differs(r, cnt, cle)) ? 1u : 0u;
        }
    }
}

// (the sets of an element of class c below: its own, and -- with classes -- "all", set ncls)

// ---- digit walk of pass 1..3: per (slot, set, rank) the histogram of the next digit among the keys with the rank's prefix
template <int V>
__global__ __launch_bounds__(kProfNT) void prof_digit_kernel(ProfArgs A) {
    ProfTile P;
    if (!prof_tile(A, P)) return;
    const int tid = threadIdx.x, nset = P.tw * A.Q, shift = 24 - 8 * A.pass;
    unsigned *hist = prof_lds;                    // [tw][Q][3][256]
    unsigned *pre = hist + nset * 3 * 256;        // [tw][Q][3]: the prefix an open rank follows
    unsigned *open = pre + nset * 3;              // [tw][Q][3], then one word: any open
    for (int i = tid; i < nset * 3 * 256 + nset * 6 + 1; i += kProfNT) prof_lds[i] = 0u;
    __syncthreads();
    for (int i = tid; i < nset * 3; i += kProfNT) {
        const int ls = i / 3, e = i - 3 * ls, tt = ls / A.Q, q = ls - tt * A.Q;
        const ProfState &st = A.st[prof_cell(A, P, q, tt)];
        pre[i] = st.ans[e] >> (shift + 8); open[i] = st.open[e];
        if (st.open[e]) open[nset * 3] = 1u;
    }
    __syncthreads();
    if (!open[nset * 3]) return;                  // (uniform: every rank of the tile is settled)
    prof_walk<V>(A, P.s, P.t0, P.tw, P.i0, P.i1, [&](int, unsigned key, double, int kind, int c, int tt, int64_t) {
        const bool ok = kind > kPcBad;
        const unsigned pk = key >> (shift + 8), d = (key >> shift) & 0xFFu;
        for (int k = 0; k < (A.Q > A.ncls ? 2 : 1); ++k) {
            const int ls = tt * A.Q + (k ? A.ncls : (c < 0 ? 0 : c));
#pragma unroll
            for (int e = 0; e < 3; ++e)
                conv_add(hist, ok && open[ls * 3 + e] && pk == pre[ls * 3 + e], (unsigned)((ls * 3 + e) * 256) + d);
        }
    });
    __syncthreads();
    for (int i = tid; i < nset * 3 * 256; i += kProfNT) {
        const unsigned v = hist[i];
        if (v) {
            const int le = i >> 8, ls = le / 3, e = le - 3 * ls, tt = ls / A.Q, q = ls - tt * A.Q;
            atomicAdd(A.hg + ((prof_cell(A, P, q, tt) * 3 + e) << 8) + (i & 255), v);
        }
    }
}

// ---- the small walks: A.pass 0: neighbours and the worst entry, 1: whisker candidates, 2: fliers
template <int V>
__global__ __launch_bounds__(kProfNT) void prof_scan_kernel(ProfArgs A) {
    ProfTile P;
    if (!prof_tile(A, P)) return;
    const int tid = threadIdx.x, nset = P.tw * A.Q;
    unsigned *a = prof_lds;                       // [tw][Q][4]: what the walk reads as integers
    unsigned *o = a + nset * 4;                   // [tw][Q][4]: what it maximises / counts; then one word: anything to do
    double *lim = reinterpret_cast<double *>(o + nset * 4 + 2);   // [tw][Q][2]
    for (int i = tid; i < nset * 8 + 2; i += kProfNT) prof_lds[i] = 0u;
    __syncthreads();
    for (int ls = tid; ls < nset; ls += kProfNT) {
        const int tt = ls / A.Q, q = ls - tt * A.Q;
        const ProfState &st = A.st[prof_cell(A, P, q, tt)];
        if (A.pass == 0) {
            for (int e = 0; e < 3; ++e) a[ls * 4 + e] = st.need[e] ? st.ans[e] : 0xFFFFFFFFu;   // (no key is above it)
            a[ls * 4 + 3] = st.count ? st.ext_hi : 0u;
            if (st.count) o[nset * 4] = 1u;
        } else if (A.pass == 1) {
            lim[ls * 2] = st.lim[0]; lim[ls * 2 + 1] = st.lim[1];
            if (st.count) o[nset * 4] = 1u;
        } else {
            lim[ls * 2] = st.w[0]; lim[ls * 2 + 1] = st.w[1];
            a[ls * 4] = st.any_fl;
            if (st.any_fl) o[nset * 4] = 1u;
        }
    }
    __syncthreads();
    if (!o[nset * 4]) return;                     // (uniform)
    const int pass = A.pass;
    prof_walk<V>(A, P.s, P.t0, P.tw, P.i0, P.i1, [&](int, unsigned key, double v, int kind, int c, int tt, int64_t i) {
        const bool ok = kind > kPcBad;
        for (int k = 0; k < (A.Q > A.ncls ? 2 : 1); ++k) {
            const int ls = tt * A.Q + (k ? A.ncls : (c < 0 ? 0 : c));
            if (pass == 0) {
                if (ok) {
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (key > a[ls * 4 + e] && ~key > o[ls * 4 + e]) atomicMax(&o[ls * 4 + e], ~key);
                    if (A.part && key == a[ls * 4 + 3]) {      // (pools take the worst entry from their members)
                        const unsigned code = 0x7FFFFFFFu - (unsigned)(A.index ? A.index[i] : (int)i);
                        if (code > o[ls * 4 + 3]) atomicMax(&o[ls * 4 + 3], code);
                    }
                }
            } else if (pass == 1) {
                if (ok) {
                    if (v >= lim[ls * 2] && ~key > o[ls * 4]) atomicMax(&o[ls * 4], ~key);
                    if (v <= lim[ls * 2 + 1] && key > o[ls * 4 + 1]) atomicMax(&o[ls * 4 + 1], key);
                }
            } else {
                conv_add(o, ok && a[ls * 4] && box_is_flier(v, lim[ls * 2], lim[ls * 2 + 1]), (unsigned)(ls * 4));
            }
        }
    });
    __syncthreads();
    for (int i = tid; i < nset * 4; i += kProfNT) {
        const unsigned v = o[i];
        if (!v) continue;
        const int ls = i >> 2, e = i & 3, tt = ls / A.Q, q = ls - tt * A.Q;
        ProfState &st = A.st[prof_cell(A, P, q, tt)];
        if (pass == 0) atomicMax(e < 3 ? &st.nb_inv[e] : &st.worst, v);
        else if (pass == 1) { if (e < 2) atomicMax(e ? &st.wk_hi : &st.wk_lo_inv, v); }
        else if (e == 0) atomicAdd(&st.fl, v);
    }
}

// ---- between the small walks, one thread per cell: A.pass 0: quartiles and whisker limits, 1: whiskers, any flier
__global__ __launch_bounds__(256) void prof_cell_kernel(ProfArgs A, int64_t ncell) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= ncell) return;
    ProfState &st = A.st[cell];
    if (!st.count) return;
    if (A.pass == 0) {
        for (int e = 0; e < 3; ++e) {
            const double lo = box_val_f(st.ans[e]);
            const double hi = st.need[e] ? box_val_f(~st.nb_inv[e]) : lo;
            st.q[e] = box_quartile(lo, hi, st.rem4[e]);
        }
        box_limits(st.q[0], st.q[2], st.lim[0], st.lim[1]);
    } else {
        const double q1 = st.q[0], q3 = st.q[2];
        const unsigned k0 = ~st.wk_lo_inv, k1 = st.wk_hi;
        const double wlo = box_whisker_lo(q1, k0 != 0xFFFFFFFFu, box_val_f(k0));
        const double whi = box_whisker_hi(q3, k1 != 0u, box_val_f(k1));
        st.w[0] = wlo; st.w[1] = whi;
        st.any_fl = (box_val_f(~st.ext_lo_inv) < wlo || box_val_f(st.ext_hi) > whi) ? 1u : 0u;
    }
}

// ---- the records: one wavefront per cell
__global__ __launch_bounds__(64) void prof_finish_kernel(ProfArgs A) {
    const int64_t cell = blockIdx.x;
    const int lane = threadIdx.x, t = (int)(cell % A.T), q = (int)((cell / A.T) % A.Q);
    const int64_t grp = cell / ((int64_t)A.T * A.Q);
    const ProfState &st = A.st[cell];
    const double nan = __builtin_nan("");
    revs_bill_summary_t r;
    r.min = r.q1 = r.median = r.q3 = r.max = r.whisker_lo = r.whisker_hi = r.total = nan;
    r.reserved0 = 0.0;
    r.count = (int)st.count; r.n_nan = (int)st.cnt[kPcBad]; r.n_fliers = 0; r.n_above = (int)st.cnt[kPcAbove];
    r.worst_index = r.worst_scenario = -1;
    if (r.count) {
        r.min = box_val_f(~st.ext_lo_inv); r.max = box_val_f(st.ext_hi);
        r.q1 = st.q[0]; r.median = st.q[1]; r.q3 = st.q[2];
        r.whisker_lo = st.w[0]; r.whisker_hi = st.w[1];
        r.n_fliers = (int)st.fl;
        if (A.part) {
            // total: per class the chunks' partials in 64 interleaved runs, chunks ascending, then the wavefront's
            // butterfly; "all": the classes' totals in class order -- the bits of the classes' own records
            const bool all = q >= A.ncls;
            bool first = true;
            for (int c = all ? 0 : q; c < (all ? A.ncls : q + 1); ++c) {
                double acc = 0.0;
                for (int ch = lane; ch < A.nchunks; ch += 64)
                    acc = acc + A.part[(((int64_t)ch * A.S + grp) * A.ncls + c) * A.T + t];
                acc = wave_sum_d(acc);
                if (A.st[(grp * A.Q + c) * A.T + t].count) { r.total = first ? acc : r.total + acc; first = false; }
            }
            r.worst_index = 0x7FFFFFFF - (int)st.worst; r.worst_scenario = (int)grp;
        } else {
            // total and the worst entry from the members' records, scenarios ascending: the largest value, then the
            // lowest scenario, then (the record's rule) the lowest index
            bool first = true;
            double best = 0.0;
            for (int s = 0; s < A.S; ++s) {
                if (A.group_of[s] != (int)grp) continue;
                const revs_bill_summary_t m = A.member[((int64_t)s * A.Q + q) * A.T + t];
                if (!m.count) continue;
                r.total = first ? m.total : r.total + m.total;
                if (first || m.max > best) { best = m.max; r.worst_index = m.worst_index; r.worst_scenario = s; }
                first = false;
            }
        }
    }
    if (lane == 0) A.out[cell] = r;
}

// ---- each residence's own daily peak: peaks[s][i] = max over t, a NaN where the row holds a value that is not finite.
// L lanes per row, consecutive lanes on consecutive slots.
struct ProfRowArgs {
    const float *g;
    float *peaks;                                 // [S][n]
    int64_t n, stride_s, stride_i, rows;
    int32_t S, T, L;
};
__global__ __launch_bounds__(256) void prof_rows_kernel(ProfRowArgs A) {
    const int64_t th = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = th / A.L;
    const int l = (int)(th - row * A.L);
    unsigned best = 0u, bad = 0u;
    int64_t i = 0, s = 0;
    if (row < A.rows) {
        i = row / A.S; s = row - i * A.S;
        const float *p = A.g + i * A.stride_i + s * A.stride_s;
        for (int t = l; t < A.T; t += A.L) {
            const unsigned u = __float_as_uint(p[t]);
            if ((u & 0x7F800000u) == 0x7F800000u) bad = 1u;
            else best = max(best, box_key_f(u));
        }
    }
    for (int o = 1; o < A.L; o <<= 1) {
        best = max(best, (unsigned)__shfl_xor((int)best, o));
        bad |= (unsigned)__shfl_xor((int)bad, o);
    }
    if (row < A.rows && l == 0) A.peaks[s * A.n + i] = bad ? __builtin_nanf("") : (float)box_val_f(best);
}

// ---- the day figures of every (scenario, set) from the records the call wrote
struct ProfDayArgs {
    const revs_bill_summary_t *slot, *peak;       // [S][Q][T], [S][Q]
    revs_profile_day_t *out;
    int32_t rows, T;
};
__global__ __launch_bounds__(256) void prof_day_kernel(ProfDayArgs A) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= A.rows) return;
    const double nan = __builtin_nan("");
    revs_profile_day_t d;
    d.peak = d.valley = d.energy = d.load_factor = d.sum_peaks = d.diversity = nan;
    d.peak_slot = d.valley_slot = -1; d.slots = 0; d.reserved = 0;
    double energy = 0.0;
    for (int t = 0; t < A.T; ++t) {
        const revs_bill_summary_t &m = A.slot[(int64_t)r * A.T + t];
        if (!m.count) continue;
        if (!d.slots || m.total > d.peak) { d.peak = m.total; d.peak_slot = t; }
        if (!d.slots || m.total < d.valley) { d.valley = m.total; d.valley_slot = t; }
        energy = energy + m.total;
        ++d.slots;
    }
    if (d.slots) {
        d.energy = energy;
        d.load_factor = (energy / (double)d.slots) / d.peak;
        d.sum_peaks = A.peak[r].total;
        d.diversity = d.sum_peaks / d.peak;
    }
    A.out[r] = d;
}

// ---- the scenario -> group table, 256 entries per launch through the kernel's arguments (the call only enqueues)
struct ProfTableArgs { int32_t *table; int32_t s0, count; int32_t id[256]; };
__global__ __launch_bounds__(256) void prof_table_kernel(ProfTableArgs A) {
    if ((int)threadIdx.x < A.count) A.table[A.s0 + threadIdx.x] = A.id[threadIdx.x];
}

}  // namespace revs

using namespace revs;

static int64_t up16(int64_t b) { return (b + 15) / 16 * 16; }

// slots of a walk workgroup's tile: what kProfHists histograms hold at 3 per (slot, set), a multiple of 4 below T
static int prof_tile_slots(int T, int Q) {
    int tt = kProfHists / (3 * Q);
    tt -= tt % 4;
    return T <= tt ? T : tt;
}

struct ProfLayout {
    int64_t state, h0, hg, zeroed, part, peaks, table, slot_rec, peak_rec, total;
};
static bool prof_layout(int32_t S, int64_t n, int32_t T, int32_t C, int32_t G, ProfLayout &L) {
    if (!(study_sizes_ok(S, n) && T >= 1 && T <= REVS_MAX_T && C >= 0 && C <= REVS_PROFILE_MAX_CLASSES && G >= 0 && G <= S))
        return false;
    const int64_t ncls = C ? C : 1, Q = C + 1, NG = S > G ? S : G, chunks = (n + kProfChunk - 1) / kProfChunk;
    L.state = 0;
    L.h0 = up16(NG * Q * T * (int64_t)sizeof(ProfState));
    L.hg = L.h0 + NG * ncls * T * 1024;
    L.zeroed = L.hg + NG * Q * T * 3 * 1024;
    L.part = L.zeroed;
    L.peaks = L.part + up16(chunks * S * ncls * T * 8);
    L.table = L.peaks + up16((int64_t)S * n * 4);
    L.slot_rec = L.table + up16((int64_t)S * 4);
    L.peak_rec = L.slot_rec + (int64_t)S * Q * T * (int64_t)sizeof(revs_bill_summary_t);
    L.total = L.peak_rec + (int64_t)S * Q * (int64_t)sizeof(revs_bill_summary_t);
    return true;
}

extern "C" int32_t revs_load_profile_chunk(void) { return kProfChunk; }

extern "C" int64_t revs_load_profile_scratch(int32_t S, int64_t n, int32_t T, int32_t C, int32_t G) {
    ProfLayout L;
    return prof_layout(S, n, T, C, G, L) ? L.total : 0;
}

template <int V>
static int prof_sequence(ProfArgs A, int64_t zero_bytes, hipStream_t st, const char *who) {
    const int64_t ncell = (int64_t)A.NG * A.Q * A.T;
    REVS_REQUIRE(ncell < ((int64_t)1 << 31), "%s: %lld cells, 2^31 or more", who, (long long)ncell);
    if (hipMemsetAsync(A.st, 0, (size_t)zero_bytes, st) != hipSuccess) {
        revs::set_error("%s: hipMemsetAsync failed", who);
        return REVS_ELAUNCH;
    }
    const dim3 grid((unsigned)A.nchunks, (unsigned)((A.T + A.TT - 1) / A.TT), (unsigned)A.S), block(kProfNT);
    const int tw = A.TT < A.T ? A.TT : A.T;
    size_t lds0 = (size_t)tw * A.ncls * (256 + 8 + 2) * 4;
    if (A.part && lds0 < (size_t)V * A.ncls * kProfNT * 8) lds0 = (size_t)V * A.ncls * kProfNT * 8;
    const size_t ldsd = ((size_t)tw * A.Q * (3 * 256 + 6) + 1) * 4, ldss = ((size_t)tw * A.Q * 8 + 2) * 4 + (size_t)tw * A.Q * 16;
    if (!grant_lds(reinterpret_cast<const void *>(&prof_pass0_kernel<V>), lds0, who)
        || !grant_lds(reinterpret_cast<const void *>(&prof_digit_kernel<V>), ldsd, who))
        return REVS_ELAUNCH;
    A.pass = 0;
    hipLaunchKernelGGL(prof_pass0_kernel<V>, grid, block, lds0, st, A);
    REVS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(prof_pick_kernel, dim3((unsigned)ncell), dim3(64), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    for (int pass = 1; pass < 4; ++pass) {
        A.pass = pass;
        hipLaunchKernelGGL(prof_digit_kernel<V>, grid, block, ldsd, st, A);
        REVS_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(prof_pick_kernel, dim3((unsigned)ncell), dim3(64), 0, st, A);
        REVS_CHECK_LAUNCH(who);
    }
    for (int pass = 0; pass < 3; ++pass) {
        A.pass = pass;
        hipLaunchKernelGGL(prof_scan_kernel<V>, grid, block, ldss, st, A);
        REVS_CHECK_LAUNCH(who);
        if (pass < 2) {
            hipLaunchKernelGGL(prof_cell_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, A, ncell);
            REVS_CHECK_LAUNCH(who);
        }
    }
    hipLaunchKernelGGL(prof_finish_kernel, dim3((unsigned)ncell), dim3(64), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    return REVS_OK;
}

extern "C" int revs_load_profile(int32_t S, int64_t n, int32_t T, const float *g, int64_t stride_s, int64_t stride_i,
                                 const uint8_t *cls, int32_t C, const int32_t *index_of_row, const int32_t *groups,
                                 int32_t G, double above, revs_bill_summary_t *slot_rec, revs_bill_summary_t *peak_rec,
                                 revs_profile_day_t *day_rec, revs_bill_summary_t *pool_slot_rec,
                                 revs_bill_summary_t *pool_peak_rec, void *scratch, void *stream) {
    static_assert(sizeof(revs_bill_summary_t) == 96 && sizeof(revs_profile_day_t) == 64, "");
    static_assert(sizeof(ProfState) % 8 == 0 && sizeof(ProfArgs) <= 4096 && sizeof(ProfTableArgs) <= 4096, "");
    static_assert((size_t)kProfHists * 1024 + 16 * 1024 <= 160 * 1024, "LDS");
    static_assert((size_t)4 * REVS_PROFILE_MAX_CLASSES * kProfNT * 8 <= 160 * 1024, "LDS");
    const char *who = "revs_load_profile";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T >= 1 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(study_sizes_ok(S, n), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(C >= 0 && C <= REVS_PROFILE_MAX_CLASSES, "%s: C=%d outside 0..%d", who, (int)C, REVS_PROFILE_MAX_CLASSES);
    REVS_REQUIRE((cls != nullptr) == (C > 0), "%s: cls and C=%d disagree (cls = NULL needs C = 0, classes need cls)", who, (int)C);
    REVS_REQUIRE(rows_inner_i(S, n, T, stride_s, stride_i) >= 0, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    REVS_REQUIRE(above == above, "%s: above is a NaN", who);
    REVS_REQUIRE(g, "%s: null pointer argument g", who);
    REVS_REQUIRE(G >= 0 && G <= S, "%s: G=%d outside 0..S=%d", who, (int)G, (int)S);
    REVS_REQUIRE(G == 0 || groups, "%s: groups is NULL with G > 0", who);
    for (int s = 0; s < S && G > 0; ++s)
        REVS_REQUIRE(groups[s] >= -1 && groups[s] < G, "%s: groups[%d]=%d outside -1..G-1", who, s, (int)groups[s]);
    REVS_REQUIRE(G > 0 || (!pool_slot_rec && !pool_peak_rec), "%s: a pool output with G == 0", who);
    REVS_REQUIRE(scratch, "%s: null pointer argument scratch (revs_load_profile_scratch bytes)", who);
    REVS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    REVS_REQUIRE(slot_rec || peak_rec || day_rec || pool_slot_rec || pool_peak_rec, "%s: every output is NULL", who);
    ProfLayout L;
    REVS_REQUIRE(prof_layout(S, n, T, C, G, L), "%s: no scratch layout for these sizes", who);

    hipStream_t st = (hipStream_t)stream;
    char *sc = (char *)scratch;
    const bool want_slot = slot_rec || day_rec || pool_slot_rec, want_peak = peak_rec || day_rec || pool_peak_rec;
    revs_bill_summary_t *srec = slot_rec ? slot_rec : (revs_bill_summary_t *)(sc + L.slot_rec);
    revs_bill_summary_t *prec = peak_rec ? peak_rec : (revs_bill_summary_t *)(sc + L.peak_rec);
    float *peaks = (float *)(sc + L.peaks);
    int32_t *table = (int32_t *)(sc + L.table);
    const bool pools = pool_slot_rec || pool_peak_rec;
    if (pools) {
        ProfTableArgs TA;
        TA.table = table;
        for (int s0 = 0; s0 < S; s0 += 256) {
            TA.s0 = s0; TA.count = S - s0 < 256 ? S - s0 : 256;
            for (int k = 0; k < 256; ++k) TA.id[k] = k < TA.count ? groups[s0 + k] : -1;
            hipLaunchKernelGGL(prof_table_kernel, dim3(1), dim3(256), 0, st, TA);
            REVS_CHECK_LAUNCH(who);
        }
    }
    if (want_peak) {
        ProfRowArgs R;
        R.g = g; R.peaks = peaks; R.n = n; R.stride_s = stride_s; R.stride_i = stride_i; R.rows = (int64_t)S * n;
        R.S = S; R.T = T; R.L = 1;
        while (R.L < T && R.L < 64) R.L *= 2;
        const int64_t blocks = (R.rows * R.L + 255) / 256;
        REVS_REQUIRE(blocks < ((int64_t)1 << 31), "%s: %lld workgroups of the row kernel, 2^31 or more", who, (long long)blocks);
        hipLaunchKernelGGL(prof_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, R);
        REVS_CHECK_LAUNCH(who);
    }
    ProfArgs A;
    A.cls = cls; A.index = index_of_row; A.st = (ProfState *)(sc + L.state); A.h0 = (unsigned *)(sc + L.h0);
    A.hg = (unsigned *)(sc + L.hg); A.n = n; A.above = above; A.S = S; A.ncls = C ? C : 1; A.Q = C + 1;
    A.nchunks = (int32_t)((n + kProfChunk - 1) / kProfChunk); A.pass = 0;
    const bool vec = T % 4 == 0 && ((uintptr_t)g & 15) == 0 && stride_s % 4 == 0 && stride_i % 4 == 0;
    for (int pool = 0; pool < (pools ? 2 : 1); ++pool) {
        A.group_of = pool ? table : nullptr; A.NG = pool ? G : S;
        A.part = pool ? nullptr : (double *)(sc + L.part);
        if (pool ? pool_slot_rec != nullptr : want_slot) {
            A.g = g; A.stride_s = stride_s; A.stride_i = stride_i; A.T = T; A.TT = prof_tile_slots(T, A.Q);
            A.member = srec; A.out = pool ? pool_slot_rec : srec;
            const int rc = vec ? prof_sequence<4>(A, L.zeroed, st, who) : prof_sequence<1>(A, L.zeroed, st, who);
            if (rc != REVS_OK) return rc;
        }
        if (pool ? pool_peak_rec != nullptr : want_peak) {
            A.g = peaks; A.stride_s = n; A.stride_i = 1; A.T = 1; A.TT = 1;
            A.member = prec; A.out = pool ? pool_peak_rec : prec;
            const int rc = prof_sequence<1>(A, L.zeroed, st, who);
            if (rc != REVS_OK) return rc;
        }
    }
    if (day_rec) {
        ProfDayArgs D;
        D.slot = srec; D.peak = prec; D.out = day_rec; D.rows = S * (C + 1); D.T = T;
        hipLaunchKernelGGL(prof_day_kernel, dim3((unsigned)((D.rows + 255) / 256)), dim3(256), 0, st, D);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}
