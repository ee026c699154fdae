// The flexibility report (include/revs_admm_ops.h, "flexibility report"): how much of a schedule's
// charging can still be moved, per EV, node and slot, from the charger power where it lies.
//
//   flex_rows_kernel<VEC>  charge_kernels.hip's row pass: a workgroup owns 256 rows of ONE scenario (grid.y) and walks the
//                          slots in chunks of 32 staged in LDS by loads that run along the rows (VEC: 16 bytes a lane,
//                          else 4), rows without an EV are never read; thread r steps row r through the chunk in slot
//                          order with done(t) in a register, so the report is one pass over p.  The chunk is stepped four
//                          slots at a time: thread r writes its up and down of the four slots into a tile of doubles
//                          (row stride 9: a half wavefront on all banks), the wavefronts ballot the slot's three
//                          conditions into LDS counters, and thread (group q, column c) adds column c of rows 8 q ..
//                          8 q + 7 in row order; one thread a column adds the 32 groups in order into the workgroup's row
//                          of partial sums.  The chunk ends with one global integer atomic per (slot, counter) that is
//                          not zero.
//                          Node sums (asked for with node_ptr): the same thread (q, c) rounds its eight values with
//                          revs_q36, adds the consecutive rows of a node and leaves each run's sum in the run's first
//                          cell; the runs that do not begin their node are added to the cell of the node's first row of
//                          the workgroup (LDS adds), and that row adds the cell into the zeroed output: one global f64
//                          add per (workgroup, node, slot) that is not zero.  Every one of these additions is exact
//                          (multiples of 2^-36 below 2^17), so their order does not show in the bits.
//   flex_fold_kernel       the partial sums are 2 T columns a workgroup (up, then down).  A fold workgroup owns 32 slots
//                          of one scenario: thread (segment, slot) adds the segment's workgroups -- a contiguous 32nd of
//                          them -- in order for both columns, then one thread a slot adds the 32 segments in order and
//                          writes the slot record.
//   flex_day_kernel        one workgroup per scenario scans the folded slots for the day record.
#include "common.h"

#include <math.h>

// every product and sum is rounded on its own (bill_kernels.hip's note on the pragma holds here too)
#pragma clang fp contract(off)

namespace revs {

constexpr int kFlxNT = 256;                       // rows of a tile: one thread each
constexpr int kFlxTC = 32;                        // slots of a chunk: 128 bytes of a row
constexpr int kFlxLD = kFlxTC + 1;
constexpr int kFlxSub = 4;                        // slots of a step
constexpr int kFlxCols = 2 * kFlxSub;             // columns of the tile of doubles: up of the step's slots, then down
constexpr int kFlxVLD = kFlxCols + 1;
constexpr int kFlxGroups = kFlxNT / kFlxCols;     // groups of consecutive rows a column is added in
constexpr int kFlxRows = kFlxNT / kFlxGroups;     // rows of a group
constexpr int kFlxSlotC = 4;                      // slot counters: plugged, up, down (4: 16 bytes)
constexpr int kFlxDayC = 8;                       // day counters: n_ev, never ready, unservable, late, rigid (8: 32 bytes)
static_assert(kFlxRows == 8 && kFlxGroups == 32 && kFlxTC % kFlxSub == 0, "");

struct FlexArgs {
    const float *p;
    const revs_home_t *homes;
    const int64_t *node_ptr;
    revs_flex_row_t *row_rec;
    int32_t *hist;
    double *node_up, *node_down, *val_out;
    uint8_t *keep_out;
    int32_t *slotc;                               // scratch int32[S][T][kFlxSlotC]
    int32_t *dayc;                                // scratch int32[S][kFlxDayC]
    double *ppart;                                // scratch double[S][nwg][2 T]: the slots' up, then their down
    int64_t stride_s, stride_i;
    double on_frac, short_tol;
    uint32_t n, S, nwg;
    int32_t T, m, integral;
};

template <bool VEC>
__global__ __launch_bounds__(kFlxNT) void flex_rows_kernel(FlexArgs A) {
    __shared__ float tile[kFlxNT * kFlxLD];
    __shared__ double vt[kFlxNT * kFlxVLD];       // [row][up of the step's slots, down of them]
    __shared__ double colpart[kFlxGroups][kFlxCols];
    __shared__ int act[kFlxNT];                   // the row is there and has an EV
    __shared__ int nd[kFlxNT];                    // the row's node, -1: none
    __shared__ int hd[kFlxNT];                    // the first row of the workgroup that has the row's node
    __shared__ int wcnt[kFlxNT / 64][kFlxTC][kFlxSlotC];
    __shared__ int dcnt[kFlxDayC];
    __shared__ int lhist[2 * (REVS_MAX_T + 1)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = A.T;
    const uint32_t s = blockIdx.y, i0 = (uint32_t)blockIdx.x * kFlxNT, i = i0 + (uint32_t)tid;
    const bool there = i < A.n;
    const bool nodes = A.node_up != nullptr;
    revs_home_t h;
    h.ev = 0; h.start = h.end = h.nmin = h.nmax = 0; h.rating = h.capacity = h.initial = 0.0f;
    if (there) h = A.homes[(int64_t)i * A.S + s];
    const bool ev = there && h.ev != 0;
    act[tid] = ev ? 1 : 0;
    if (tid < kFlxDayC) dcnt[tid] = 0;
    if (A.hist)
        for (int k = tid; k < 2 * (T + 1); k += kFlxNT) lhist[k] = 0;
    if (nodes) {                                  // the node j with node_ptr[j] <= i < node_ptr[j + 1]
        int node = -1, head = tid;
        if (there) {
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
    const int ws = h.start < 0 ? 0 : h.start > T ? T : h.start, we = h.end < 0 ? 0 : h.end > T ? T : h.end;
    const int W = we - ws > 0 ? we - ws : 0;
    const double r = (double)h.rating, c = (double)h.capacity, ini = (double)h.initial, thr = A.on_frac * r;
    const double tgt = ini > 0.9 ? ini : 0.9;
    const double E_lo = (tgt - ini) * c, E_hi = (1.0 - ini) * c;
    const float *base = A.p + (int64_t)s * A.stride_s + (int64_t)i0 * A.stride_i;
    const int rows_here = A.n - i0 < (uint32_t)kFlxNT ? (int)(A.n - i0) : kFlxNT;

    double done = 0.0, up_energy = 0.0, down_energy = 0.0;
    int n_up = 0, n_down = 0;
    int ready = ev && !(tgt - (ini + done / c) > A.short_tol) ? 0 : -1;
    bool bad = false;
    for (int c0 = 0; c0 < T; c0 += kFlxTC) {
        __syncthreads();                          // (act is visible; the chunk before is read)
        if (VEC) {
#pragma unroll
            for (int k = 0; k < kFlxTC / 4; ++k) {   // piece e of the tile's chunk: row e / 8, slots c0 + 4 (e % 8) ..
                const int e = k * kFlxNT + tid, rr = e / (kFlxTC / 4), t = 4 * (e % (kFlxTC / 4));
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rr < rows_here && act[rr]) {
                    const float *src = base + (int64_t)rr * A.stride_i + c0 + t;
                    if (c0 + t + 3 < T) x = *reinterpret_cast<const float4 *>(src);
                    else {
                        if (c0 + t < T) x.x = src[0];
                        if (c0 + t + 1 < T) x.y = src[1];
                        if (c0 + t + 2 < T) x.z = src[2];
                    }
                }
                float *dst = tile + rr * kFlxLD + t;
                dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
            }
        } else {
#pragma unroll 8
            for (int k = 0; k < kFlxTC; ++k) {    // element e of the tile's chunk: row e / 32, slot c0 + e % 32
                const int e = k * kFlxNT + tid, rr = e / kFlxTC, t = e % kFlxTC;
                float x = 0.f;
                if (rr < rows_here && act[rr] && c0 + t < T) x = base[(int64_t)rr * A.stride_i + c0 + t];
                tile[rr * kFlxLD + t] = x;
            }
        }
        __syncthreads();
        const int tc = T - c0 < kFlxTC ? T - c0 : kFlxTC;
        const float *row = tile + tid * kFlxLD;
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
                    const unsigned long long b0 = __ballot(plugged), b1 = __ballot(up > 0.0), b2 = __ballot(down > 0.0);
                    if (lane == 0) {
                        wcnt[wave][j][0] = __popcll(b0); wcnt[wave][j][1] = __popcll(b1); wcnt[wave][j][2] = __popcll(b2);
                    }
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
                    A.ppart[((int64_t)s * A.nwg + blockIdx.x) * (2 * (int64_t)T) + (int64_t)which * T + c0 + j0 + jj] = acc;
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
        if (tid >= 128 && tid - 128 < tc * kFlxSlotC) {
            const int j = (tid - 128) / kFlxSlotC, cc = (tid - 128) % kFlxSlotC;
            if (cc < 3) {
                int v = 0;
#pragma unroll
                for (int w = 0; w < kFlxNT / 64; ++w) v += wcnt[w][j][cc];
                if (v) atomicAdd(A.slotc + ((int64_t)s * T + c0 + j) * kFlxSlotC + cc, v);
            }
        }
    }

    // ---- the row's record
    const double laxity = (double)W - E_lo / r;
    const bool never = ev && ready < 0, unserv = ev && E_lo > (double)W * r, late = ev && ready > we;
    const int slack = ready >= 0 ? we - ready : 0;
    const int64_t out = (int64_t)s * A.n + i;
    if (there) {
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
            const int64_t plane = (int64_t)A.S * A.n;
            A.val_out[out] = keep ? up_energy : nan;
            A.val_out[plane + out] = keep ? down_energy : nan;
            A.val_out[2 * plane + out] = keep && ready >= 0 ? (double)slack : nan;
            A.val_out[3 * plane + out] = keep ? laxity : nan;
        }
        if (A.keep_out) A.keep_out[out] = keep ? 1 : 0;
    }
    // ---- the workgroup's share of the day record and of the histograms
    {
        const unsigned long long b0 = __ballot(ev), b1 = __ballot(never), b2 = __ballot(unserv), b3 = __ballot(late),
                                 b4 = __ballot(ev && n_up == 0 && n_down == 0);
        if (lane == 0) {
            if (b0) atomicAdd(&dcnt[0], __popcll(b0));
            if (b1) atomicAdd(&dcnt[1], __popcll(b1));
            if (b2) atomicAdd(&dcnt[2], __popcll(b2));
            if (b3) atomicAdd(&dcnt[3], __popcll(b3));
            if (b4) atomicAdd(&dcnt[4], __popcll(b4));
        }
    }
    if (A.hist && ev && ready >= 0) {
        atomicAdd(&lhist[ready], 1);
        if (slack >= 0 && slack <= T) atomicAdd(&lhist[(T + 1) + slack], 1);
    }
    __syncthreads();
    if (tid >= 64 && tid < 64 + kFlxDayC && dcnt[tid - 64]) atomicAdd(A.dayc + (int64_t)s * kFlxDayC + (tid - 64), dcnt[tid - 64]);
    if (A.hist)
        for (int k = tid; k < 2 * (T + 1); k += kFlxNT)
            if (lhist[k]) atomicAdd(A.hist + (int64_t)s * 2 * (T + 1) + k, lhist[k]);
}

constexpr int kFlxFoldSeg = 32;                   // chains a column's workgroups are folded in
constexpr int kFlxFoldCols = 32;                  // slots of a fold workgroup

struct FlexFoldArgs {
    const int32_t *slotc, *dayc;
    const double *ppart;
    double *folded;                               // scratch double[S][2 T]
    revs_flex_slot_t *slot_rec;
    revs_flex_day_t *day_rec;
    uint32_t nwg;
    int32_t T;
};

__global__ __launch_bounds__(kFlxFoldSeg * kFlxFoldCols) void flex_fold_kernel(FlexFoldArgs A) {
    __shared__ double part[2][kFlxFoldSeg][kFlxFoldCols + 1];
    const int tid = threadIdx.x, lane = tid % kFlxFoldCols, seg = tid / kFlxFoldCols;
    const int T = A.T, t = (int)blockIdx.x * kFlxFoldCols + lane;
    const int64_t s = blockIdx.y, C = 2 * (int64_t)T;
    const uint32_t len = (A.nwg + kFlxFoldSeg - 1) / kFlxFoldSeg;
    const uint32_t w0 = (uint32_t)seg * len, w1 = w0 + len < A.nwg ? w0 + len : A.nwg;
    double up = 0.0, down = 0.0;
    if (t < T) {
        const double *pp = A.ppart + s * A.nwg * C + t;
        for (uint32_t w = w0; w < w1; ++w) {
            up = up + pp[(int64_t)w * C];
            down = down + pp[(int64_t)w * C + T];
        }
    }
    part[0][seg][lane] = up; part[1][seg][lane] = down;
    __syncthreads();
    if (seg != 0 || t >= T) return;
    up = 0.0; down = 0.0;
#pragma unroll 8
    for (int q = 0; q < kFlxFoldSeg; ++q) {
        up = up + part[0][q][lane];
        down = down + part[1][q][lane];
    }
    A.folded[s * C + t] = up;
    A.folded[s * C + T + t] = down;
    if (A.slot_rec) {
        const int32_t *cnt = A.slotc + (s * T + t) * kFlxSlotC;
        revs_flex_slot_t o;
        o.n_plugged = cnt[0]; o.n_up = cnt[1]; o.n_down = cnt[2]; o.reserved = 0;
        o.up = up; o.down = down;
        A.slot_rec[s * T + t] = o;
    }
}

__global__ __launch_bounds__(256) void flex_day_kernel(FlexFoldArgs A) {
    static_assert(REVS_MAX_T <= 256, "a thread per slot");
    __shared__ double val[2][REVS_MAX_T];
    const int tid = threadIdx.x, T = A.T;
    const int64_t s = blockIdx.x;
    if (tid < T) {
        val[0][tid] = A.folded[s * 2 * T + tid];
        val[1][tid] = A.folded[s * 2 * T + T + tid];
    }
    __syncthreads();
    if (tid != 0) return;
    const int32_t *dc = A.dayc + s * kFlxDayC;
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

static bool flex_sizes_ok(int32_t S, int64_t n, int32_t T) {
    return study_sizes_ok(S, n) && T >= 1 && T <= REVS_MAX_T;
}
static int64_t flex_int_bytes(int32_t S, int32_t T) {           // the counters in front of the scratch, a multiple of 16
    return ((int64_t)S * T * kFlxSlotC + (int64_t)S * kFlxDayC) * (int64_t)sizeof(int32_t);
}

extern "C" int32_t revs_flex_report_chunk(void) { return kFlxTC; }

extern "C" int64_t revs_flex_report_scratch(int32_t S, int64_t n, int32_t T) {
    if (!flex_sizes_ok(S, n, T)) return 0;
    const int64_t nwg = (n + kFlxNT - 1) / kFlxNT;
    const int64_t bytes = flex_int_bytes(S, T) + (int64_t)S * (nwg + 1) * (2 * (int64_t)T) * (int64_t)sizeof(double);
    return (bytes + 15) / 16 * 16;
}

extern "C" int revs_flex_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                                const revs_home_t *homes, int32_t integral, double on_frac, double short_tol,
                                const int64_t *node_ptr, int32_t m,
                                revs_flex_row_t *row_rec, revs_flex_slot_t *slot_rec, revs_flex_day_t *day_rec, int32_t *hist,
                                double *node_up, double *node_down, double *val_out, uint8_t *keep_out,
                                void *scratch, void *stream) {
    static_assert(sizeof(revs_flex_row_t) == 64 && sizeof(revs_flex_slot_t) == 32 && sizeof(revs_flex_day_t) == 64, "");
    static_assert(sizeof(revs_home_t) == 32, "");
    const char *who = "revs_flex_report";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(flex_sizes_ok(S, n, T), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(p, "%s: null pointer argument p", who);
    REVS_REQUIRE(homes, "%s: null pointer argument homes", who);
    REVS_REQUIRE(rows_inner_i(S, n, T, stride_s, stride_i) >= 0, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    REVS_REQUIRE(on_frac >= 0.0, "%s: on_frac=%g is negative or a NaN", who, on_frac);
    REVS_REQUIRE(short_tol >= 0.0, "%s: short_tol=%g is negative or a NaN", who, short_tol);
    REVS_REQUIRE(scratch, "%s: null pointer argument scratch", who);
    REVS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    REVS_REQUIRE(row_rec || slot_rec || day_rec || hist || node_up || node_down || val_out || keep_out,
                 "%s: every output is NULL", who);
    REVS_REQUIRE((node_up != nullptr) == (node_down != nullptr), "%s: node_up and node_down are asked for together", who);
    if (node_up) {
        REVS_REQUIRE(node_ptr, "%s: null pointer argument node_ptr (the node outputs need it)", who);
        REVS_REQUIRE(m >= 1, "%s: m=%d < 1 (the node outputs need the nodes)", who, (int)m);
        REVS_REQUIRE((int64_t)m * S < ((int64_t)1 << 31) / T, "%s: m*S*T cells, 2^31 or more (m=%d, S=%d, T=%d)", who,
                     (int)m, (int)S, (int)T);
    }

    hipStream_t st = (hipStream_t)stream;
    const uint32_t nwg = (uint32_t)((n + kFlxNT - 1) / kFlxNT);
    const int64_t ib = flex_int_bytes(S, T);
    FlexArgs A;
    A.p = p; A.homes = homes; A.node_ptr = node_ptr; A.row_rec = row_rec; A.hist = hist;
    A.node_up = node_up; A.node_down = node_down; A.val_out = val_out; A.keep_out = keep_out;
    A.slotc = (int32_t *)scratch; A.dayc = A.slotc + (int64_t)S * T * kFlxSlotC;
    double *folded = (double *)((char *)scratch + ib);
    A.ppart = folded + (int64_t)S * 2 * T;
    A.stride_s = stride_s; A.stride_i = stride_i; A.on_frac = on_frac; A.short_tol = short_tol;
    A.n = (uint32_t)n; A.S = (uint32_t)S; A.nwg = nwg; A.T = T; A.m = node_up ? m : 0; A.integral = integral;
    const size_t node_bytes = node_up ? (size_t)S * (size_t)m * (size_t)T * sizeof(double) : 0;
    if (hipMemsetAsync(scratch, 0, (size_t)ib, st) != hipSuccess
        || (hist && hipMemsetAsync(hist, 0, (size_t)S * 2 * (T + 1) * sizeof(int32_t), st) != hipSuccess)
        || (node_up && (hipMemsetAsync(node_up, 0, node_bytes, st) != hipSuccess
                        || hipMemsetAsync(node_down, 0, node_bytes, st) != hipSuccess))) {
        revs::set_error("%s: clearing the counters failed", who);
        return REVS_ELAUNCH;
    }
    const bool vec = ((uintptr_t)p & 15) == 0 && stride_s % 4 == 0 && stride_i % 4 == 0;
    const dim3 grid(nwg, (unsigned)S);
    if (vec) hipLaunchKernelGGL(flex_rows_kernel<true>, grid, dim3(kFlxNT), 0, st, A);
    else hipLaunchKernelGGL(flex_rows_kernel<false>, grid, dim3(kFlxNT), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    if (slot_rec || day_rec) {
        FlexFoldArgs F;
        F.slotc = A.slotc; F.dayc = A.dayc; F.ppart = A.ppart; F.folded = folded; F.slot_rec = slot_rec; F.day_rec = day_rec;
        F.nwg = nwg; F.T = T;
        hipLaunchKernelGGL(flex_fold_kernel, dim3((unsigned)((T + kFlxFoldCols - 1) / kFlxFoldCols), (unsigned)S),
                           dim3(kFlxFoldSeg * kFlxFoldCols), 0, st, F);
        REVS_CHECK_LAUNCH(who);
        if (day_rec) {
            hipLaunchKernelGGL(flex_day_kernel, dim3((unsigned)S), dim3(256), 0, st, F);
            REVS_CHECK_LAUNCH(who);
        }
    }
    return REVS_OK;
}
