// The flexibility report (include/revs_admm_ops.h, "flexibility report"): how much of a schedule's
// charging can still be moved, per EV, node and slot, from the charger power where it lies.
//
//   flex_rows_kernel<VEC>  rows_pass.h's row pass: thread r steps row r through the staged chunk in slot order with
//                          done(t) in a register, so the report is one pass over p.  The chunk is stepped four
//                          slots at a time: thread r writes its up and down of the four slots into a tile of doubles
//                          (row stride 9: a half wavefront on all banks), the wavefronts ballot the slot's three
//                          conditions, and thread (group q, column c) adds column c of rows 8 q .. 8 q + 7 in row
//                          order; one thread a column adds the 32 groups in order into the workgroup's row of partial
//                          sums.
//                          Node sums (asked for with node_ptr): the same thread (q, c) rounds its eight values with
//                          revs_q36, adds the consecutive rows of a node and leaves each run's sum in the run's first
//                          cell; the runs that do not begin their node are added to the cell of the node's first row of
//                          the workgroup (LDS adds), and that row adds the cell into the zeroed output: one global f64
//                          add per (workgroup, node, slot) that is not zero.  Every one of these additions is exact
//                          (multiples of 2^-36 below 2^17), so their order does not show in the bits.
//   flex_fold_kernel       the partial sums are 2 T columns a workgroup (up, then down), folded by rows_pass.h's chain
//                          two at a time, a slot's up and its down; the thread that holds them writes the slot record.
//   flex_day_kernel        one workgroup per scenario scans the folded slots for the day record.
#include "common.h"
#include "rows_pass.h"

#include <math.h>

// every product and sum is rounded on its own (bill_kernels.hip's note on the pragma holds here too)
#pragma clang fp contract(off)

namespace revs {

constexpr int kFlxSub = 4;                        // slots of a step
constexpr int kFlxCols = 2 * kFlxSub;             // columns of the tile of doubles: up of the step's slots, then down
constexpr int kFlxVLD = kFlxCols + 1;
constexpr int kFlxGroups = kRowNT / kFlxCols;     // groups of consecutive rows a column is added in
constexpr int kFlxRows = kRowNT / kFlxGroups;     // rows of a group
static_assert(kFlxRows == 8 && kFlxGroups == 32 && kRowTC % kFlxSub == 0, "");

// slot counters: plugged, up, down; day counters: n_ev, never ready, unservable, late, rigid
struct FlexArgs {
    RowsIn in;
    const int64_t *node_ptr;
    revs_flex_row_t *row_rec;
    int32_t *hist;
    double *node_up, *node_down, *val_out;
    uint8_t *keep_out;
    RowsScratch w;                                // 2 T columns: the slots' up, then their down
    double on_frac, short_tol;
    int32_t m, integral;
};

template <bool VEC>
__global__ __launch_bounds__(kRowNT) void flex_rows_kernel(FlexArgs A) {
    __shared__ float tile[kRowNT * kRowLD];
    __shared__ double vt[kRowNT * kFlxVLD];       // [row][up of the step's slots, down of them]
    __shared__ double colpart[kFlxGroups][kFlxCols];
    __shared__ int act[kRowNT];                   // the row is there and has an EV
    __shared__ int nd[kRowNT];                    // the row's node, -1: none
    __shared__ int hd[kRowNT];                    // the first row of the workgroup that has the row's node
    __shared__ int wcnt[kRowNT / 64][kRowTC][kRowSlotC];
    __shared__ int dcnt[kRowDayC];
    __shared__ int lhist[2 * (REVS_MAX_T + 1)];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int T = A.in.T;
    const RowStart R = rows_start(A.in, act);
    const revs_home_t &h = R.h;
    const uint32_t s = R.s, i = R.i, i0 = (uint32_t)blockIdx.x * kRowNT;
    const bool ev = R.ev, nodes = A.node_up != nullptr;
    const int ws = R.ws, we = R.we;
    rows_day_clear<2>(dcnt, lhist, A.hist != nullptr, T);
    if (nodes) {                                  // the node j with node_ptr[j] <= i < node_ptr[j + 1]
        int node = -1, head = tid;
        if (R.there) {
            int lo = 0, hi = A.m + 1;             // the first k in 0..m + 1 with node_ptr[k] > i (m + 1: none)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (A.node_ptr[mid] > (int64_t)i) hi = mid; else lo = mid + 1;
            }
            if (lo >= 1 && lo <= A.m) {
                node = lo - 1;
                const int64_t first = A.node_ptr[node] - (int64_t)i0;
                head = first > 0 ? (int)first : 0;
            }
        }
        nd[tid] = node; hd[tid] = head;
    }
    const int W = we - ws > 0 ? we - ws : 0;
    const double r = (double)h.rating, c = (double)h.capacity, ini = (double)h.initial, thr = A.on_frac * r;
    const double tgt = ini > 0.9 ? ini : 0.9;
    const double E_lo = (tgt - ini) * c, E_hi = (1.0 - ini) * c;

    double done = 0.0, up_energy = 0.0, down_energy = 0.0;
    int n_up = 0, n_down = 0;
    int ready = ev && !(tgt - (ini + done / c) > A.short_tol) ? 0 : -1;
    bool bad = false;
    for (int c0 = 0; c0 < T; c0 += kRowTC) {
        __syncthreads();                          // (act is visible; the chunk before is read)
        rows_stage<VEC>(tile, act, A.in, R, c0);
        __syncthreads();
        const int tc = T - c0 < kRowTC ? T - c0 : kRowTC;
        const float *row = tile + tid * kRowLD;
        for (int j0 = 0; j0 < tc; j0 += kFlxSub) {
#pragma unroll
            for (int jj = 0; jj < kFlxSub; ++jj) {
                const int j = j0 + jj, t = c0 + j;
                double up = 0.0, down = 0.0;
                bool plugged = false;
                if (j < tc) {                     // (the same for every thread)
                    if (ev) {
                        const double d = (double)row[j];
                        plugged = ws <= t && t < we;
                        if (plugged) {
                            const double a = r - d, b = (E_hi - done) - d;
                            double mm = b < a ? b : a;
                            up = mm > 0.0 ? (mm < r ? mm : r) : 0.0;
                            const int later = we - (t + 1 > ws ? t + 1 : ws);
                            mm = ((done + d) + (double)(later > 0 ? later : 0) * r) - E_lo;
                            const double q = d < r ? d : r;
                            down = mm > 0.0 && q > 0.0 ? (mm < q ? mm : q) : 0.0;
                            if (A.integral) {
                                up = up >= r ? r : 0.0;
                                down = d > thr && mm >= d && q > 0.0 ? q : 0.0;
                            }
                        }
                        bad = bad || !(d - d == 0.0);
                        done = done + d;
                        if (ready < 0 && !(tgt - (ini + done / c) > A.short_tol)) ready = t + 1;
                        up_energy = up_energy + up;
                        down_energy = down_energy + down;
                        n_up += up > 0.0 ? 1 : 0;
                        n_down += down > 0.0 ? 1 : 0;
                    }
                    rows_slot_ballot(wcnt[wave][j], {plugged, up > 0.0, down > 0.0});
                }
                vt[tid * kFlxVLD + jj] = up;
                vt[tid * kFlxVLD + kFlxSub + jj] = down;
            }
            __syncthreads();
            const int col = tid % kFlxCols, q = tid / kFlxCols;
            {   // column col of rows 8 q .. 8 q + 7 in row order (rows without an EV hold zeros)
                double v[kFlxRows], acc = 0.0;
#pragma unroll
                for (int k = 0; k < kFlxRows; ++k) {
                    v[k] = vt[(q * kFlxRows + k) * kFlxVLD + col];
                    acc = acc + v[k];
                }
                colpart[q][col] = acc;
                if (nodes) {                      // the runs of rows of one node: each run's sum into its first cell
                    int first = 0;
                    double run = revs_q36(v[0]);
#pragma unroll
                    for (int k = 1; k < kFlxRows; ++k) {
                        const int rr = q * kFlxRows + k;
                        if (nd[rr] != nd[rr - 1]) {
                            vt[(q * kFlxRows + first) * kFlxVLD + col] = run;
                            first = k;
                            run = revs_q36(v[k]);
                        } else run = run + revs_q36(v[k]);
                    }
                    vt[(q * kFlxRows + first) * kFlxVLD + col] = run;
                }
            }
            __syncthreads();
            if (tid < kFlxCols) {
                const int jj = tid % kFlxSub, which = tid / kFlxSub;
                if (j0 + jj < tc) {
                    double acc = 0.0;
#pragma unroll 8
                    for (int g = 0; g < kFlxGroups; ++g) acc = acc + colpart[g][tid];
                    A.w.ppart[((int64_t)s * A.in.nwg + blockIdx.x) * (2 * (int64_t)T) + (int64_t)which * T + c0 + j0 + jj] = acc;
                }
            }
            if (nodes) {
                // a run that does not begin its node (only one that begins a group can): into the cell of the node's
                // first row here
                {
                    const int rr = q * kFlxRows;
                    if (rr > 0 && nd[rr] >= 0 && nd[rr] == nd[rr - 1]) {
                        const double v = vt[rr * kFlxVLD + col];
                        if (v != 0.0) unsafeAtomicAdd(&vt[hd[rr] * kFlxVLD + col], v);
                    }
                }
                __syncthreads();
                const int jj = col % kFlxSub, t = c0 + j0 + jj;
                double *dst = col < kFlxSub ? A.node_up : A.node_down;
#pragma unroll
                for (int k = 0; k < kFlxRows; ++k) {
                    const int rr = q * kFlxRows + k;
                    if (nd[rr] >= 0 && hd[rr] == rr && t < T) {
                        const double v = vt[rr * kFlxVLD + col];
                        if (v != 0.0) unsafeAtomicAdd(dst + ((int64_t)s * A.m + nd[rr]) * T + t, v);
                    }
                }
                __syncthreads();                  // (the cells are read before the next step writes them)
            }
        }
        rows_slot_flush<3>(wcnt, A.w.slotc, s, T, c0, tc);
    }

    // ---- the row's record
    const double laxity = (double)W - E_lo / r;
    const bool never = ev && ready < 0, unserv = ev && E_lo > (double)W * r, late = ev && ready > we;
    const int slack = ready >= 0 ? we - ready : 0;
    const int64_t out = R.out;
    if (R.there) {
        if (A.row_rec) {
            revs_flex_row_t o;
            o.up_energy = ev ? up_energy : 0.0; o.down_energy = ev ? down_energy : 0.0;
            o.laxity = ev ? laxity : 0.0; o.energy = ev ? done : 0.0;
            o.ready = ready; o.slack = ev ? slack : 0; o.n_up = n_up; o.n_down = n_down;
            o.flags = ev ? 1 | (never ? 2 : 0) | (bad ? 4 : 0) | (unserv ? 8 : 0) | (late ? 16 : 0) : 0;
            o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
            A.row_rec[out] = o;
        }
        const bool keep = ev && !bad;
        if (A.val_out) {
            const double nan = __builtin_nan("");
            const int64_t plane = (int64_t)A.in.S * A.in.n;
            A.val_out[out] = keep ? up_energy : nan;
            A.val_out[plane + out] = keep ? down_energy : nan;
            A.val_out[2 * plane + out] = keep && ready >= 0 ? (double)slack : nan;
            A.val_out[3 * plane + out] = keep ? laxity : nan;
        }
        if (A.keep_out) A.keep_out[out] = keep ? 1 : 0;
    }
    // ---- the workgroup's share of the day record and of the histograms
    rows_day_count(dcnt, {ev, never, unserv, late, ev && n_up == 0 && n_down == 0});
    if (A.hist && ev && ready >= 0) {
        atomicAdd(&lhist[ready], 1);
        if (slack >= 0 && slack <= T) atomicAdd(&lhist[(T + 1) + slack], 1);
    }
    __syncthreads();
    rows_day_flush<2>(dcnt, lhist, A.w.dayc, A.hist, s, T);
}

using FlexFoldArgs = RowsFoldArgs<revs_flex_slot_t, revs_flex_day_t>;   // folded: double[S][2 T]

__global__ __launch_bounds__(kRowFoldSeg * kRowFoldCols) void flex_fold_kernel(FlexFoldArgs A) {
    __shared__ double part[2][kRowFoldSeg][kRowFoldCols + 1];
    const int T = A.T, t = (int)blockIdx.x * kRowFoldCols + (int)threadIdx.x % kRowFoldCols;
    const int64_t s = blockIdx.y, C = 2 * (int64_t)T;
    double acc[2];                                // the slot's up and down
    if (!rows_fold<2>(part, A.w.ppart, A.nwg, C, T, t < T, acc)) return;
    A.w.folded[s * C + t] = acc[0];
    A.w.folded[s * C + T + t] = acc[1];
    if (A.slot_rec) {
        const int32_t *cnt = A.w.slotc + (s * T + t) * kRowSlotC;
        revs_flex_slot_t o;
        o.n_plugged = cnt[0]; o.n_up = cnt[1]; o.n_down = cnt[2]; o.reserved = 0;
        o.up = acc[0]; o.down = acc[1];
        A.slot_rec[s * T + t] = o;
    }
}

__global__ __launch_bounds__(256) void flex_day_kernel(FlexFoldArgs A) {
    static_assert(REVS_MAX_T <= 256, "a thread per slot");
    __shared__ double val[2][REVS_MAX_T];
    const int tid = threadIdx.x, T = A.T;
    const int64_t s = blockIdx.x;
    if (tid < T) {
        val[0][tid] = A.w.folded[s * 2 * T + tid];
        val[1][tid] = A.w.folded[s * 2 * T + T + tid];
    }
    __syncthreads();
    if (tid != 0) return;
    const int32_t *dc = A.w.dayc + s * kRowDayC;
    const int n_ev = dc[0];
    double en[2], pk[2];
    int pks[2];
    for (int k = 0; k < 2; ++k) {
        en[k] = 0.0; pk[k] = val[k][0]; pks[k] = 0;
        for (int t = 0; t < T; ++t) {
            en[k] = en[k] + val[k][t];
            if (val[k][t] > pk[k]) { pk[k] = val[k][t]; pks[k] = t; }
        }
    }
    revs_flex_day_t d;
    d.up_energy = en[0]; d.down_energy = en[1]; d.peak_up = pk[0]; d.peak_down = pk[1];
    d.peak_up_slot = n_ev ? pks[0] : -1; d.peak_down_slot = n_ev ? pks[1] : -1;
    d.n_ev = n_ev; d.n_never_ready = dc[1]; d.n_unservable = dc[2]; d.n_late = dc[3]; d.n_rigid = dc[4]; d.reserved = 0;
    A.day_rec[s] = d;
}

}  // namespace revs

using namespace revs;

extern "C" int32_t revs_flex_report_chunk(void) { return kRowTC; }

extern "C" int64_t revs_flex_report_scratch(int32_t S, int64_t n, int32_t T) {
    return rows_scratch_bytes(S, n, T, 2 * (int64_t)T);
}

extern "C" int revs_flex_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                                const revs_home_t *homes, int32_t integral, double on_frac, double short_tol,
                                const int64_t *node_ptr, int32_t m,
                                revs_flex_row_t *row_rec, revs_flex_slot_t *slot_rec, revs_flex_day_t *day_rec, int32_t *hist,
                                double *node_up, double *node_down, double *val_out, uint8_t *keep_out,
                                void *scratch, void *stream) {
    static_assert(sizeof(revs_flex_row_t) == 64 && sizeof(revs_flex_slot_t) == 32 && sizeof(revs_flex_day_t) == 64, "");
    const char *who = "revs_flex_report";
    FlexArgs A;
    if (int rc = rows_args(who, S, n, T, p, stride_s, stride_i, homes, on_frac, short_tol, scratch,
                           row_rec || slot_rec || day_rec || hist || node_up || node_down || val_out || keep_out, &A.in))
        return rc;
    REVS_REQUIRE((node_up != nullptr) == (node_down != nullptr), "%s: node_up and node_down are asked for together", who);
    if (node_up) {
        REVS_REQUIRE(node_ptr, "%s: null pointer argument node_ptr (the node outputs need it)", who);
        REVS_REQUIRE(m >= 1, "%s: m=%d < 1 (the node outputs need the nodes)", who, (int)m);
        REVS_REQUIRE((int64_t)m * S < ((int64_t)1 << 31) / T, "%s: m*S*T cells, 2^31 or more (m=%d, S=%d, T=%d)", who,
                     (int)m, (int)S, (int)T);
    }

    hipStream_t st = (hipStream_t)stream;
    A.node_ptr = node_ptr; A.row_rec = row_rec; A.hist = hist;
    A.node_up = node_up; A.node_down = node_down; A.val_out = val_out; A.keep_out = keep_out;
    A.w = rows_scratch(scratch, S, T, 2 * (int64_t)T);
    A.on_frac = on_frac; A.short_tol = short_tol; A.m = node_up ? m : 0; A.integral = integral;
    const size_t node_bytes = node_up ? (size_t)S * (size_t)m * (size_t)T * sizeof(double) : 0;
    if (int rc = rows_clear(who, st, {{scratch, (size_t)rows_int_bytes(S, T)},
                                      {hist, (size_t)S * 2 * (T + 1) * sizeof(int32_t)},
                                      {node_up, node_bytes}, {node_down, node_bytes}}))
        return rc;
    hipLaunchKernelGGL(rows_vec_ok(A.in) ? flex_rows_kernel<true> : flex_rows_kernel<false>, dim3(A.in.nwg, (unsigned)S),
                       dim3(kRowNT), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    const FlexFoldArgs F = {A.w, slot_rec, day_rec, A.in.nwg, T};
    return rows_fold_launch(who, st, flex_fold_kernel, flex_day_kernel, F, T, S);
}
