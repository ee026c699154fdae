// The row pass of the reports that read charger power where it lies (charge_kernels.hip, flex_kernels.hip; DESIGN.md
// sections 3.14 and 3.18): what the two share, as pieces their rows kernels and fold kernels are put together from.
//
// A rows workgroup owns kRowNT = 256 rows of ONE scenario (grid.y) and walks the slots in chunks of kRowTC = 32 staged in
// LDS; thread r then steps row r through the chunk in slot order with the report's own code.  The LDS row stride is
// kRowLD = 33 words: thread r reads word 33 r + t, which spreads a half wavefront over all banks, and a walk down the
// columns reads 33 r + t with t along the lanes: consecutive banks.
//
// The __shared__ arrays are the kernels': a piece takes a pointer and is inlined, so the accesses stay LDS accesses.
// Nothing here asks which report calls it.
#pragma once

#include "common.h"

// every sum is rounded on its own (the including files set the same: bill_kernels.hip's note on the pragma)
#pragma clang fp contract(off)

namespace revs {

constexpr int kRowNT = 256;                       // rows of a tile: one thread each
constexpr int kRowTC = 32;                        // slots of a chunk: 128 bytes of a row
constexpr int kRowLD = kRowTC + 1;
constexpr int kRowSlotC = 4;                      // slot counters of a (scenario, slot): 16 bytes
constexpr int kRowDayC = 8;                       // day counters of a scenario, five in use (8: 32 bytes)
constexpr int kRowFoldSeg = 32;                   // chains a column's workgroups are folded in
constexpr int kRowFoldCols = 32;                  // columns of a fold workgroup
static_assert(sizeof(revs_home_t) == 32, "");

struct RowsIn {
    const float *p;
    const revs_home_t *homes;
    int64_t stride_s, stride_i;
    uint32_t n, S, nwg;
    int32_t T;
};

// The scratch of a report whose rows kernel leaves C columns of partial sums a workgroup; the counters come first,
// a multiple of 16 bytes together, and are cleared before the rows kernel.
struct RowsScratch {
    int32_t *slotc;                               // int32[S][T][kRowSlotC]
    int32_t *dayc;                                // int32[S][kRowDayC]
    double *folded;                               // double[S][C]
    double *ppart;                                // double[S][nwg][C]
};

struct RowStart {
    revs_home_t h;                                // zeros where the row is not there
    const float *base;                            // row 0 of the tile, slot 0
    int64_t out;                                  // the row's place in an [S][n] output
    uint32_t s, i;
    int ws, we, rows_here;                        // the window clamped to 0..T; the tile's rows that are there
    bool there, ev;
};

// Thread tid's row of the tile; act[tid]: the row is there and has an EV (visible after the next barrier).
__device__ __forceinline__ RowStart rows_start(const RowsIn &A, int *act) {
    const int tid = threadIdx.x, T = A.T;
    const uint32_t i0 = (uint32_t)blockIdx.x * kRowNT;
    RowStart R;
    R.s = blockIdx.y; R.i = i0 + (uint32_t)tid;
    R.there = R.i < A.n;
    R.h.ev = 0; R.h.start = R.h.end = R.h.nmin = R.h.nmax = 0; R.h.rating = R.h.capacity = R.h.initial = 0.0f;
    if (R.there) R.h = A.homes[(int64_t)R.i * A.S + R.s];
    R.ev = R.there && R.h.ev != 0;
    act[tid] = R.ev ? 1 : 0;
    R.ws = R.h.start < 0 ? 0 : R.h.start > T ? T : R.h.start;
    R.we = R.h.end < 0 ? 0 : R.h.end > T ? T : R.h.end;
    R.base = A.p + (int64_t)R.s * A.stride_s + (int64_t)i0 * A.stride_i;
    R.rows_here = A.n - i0 < (uint32_t)kRowNT ? (int)(A.n - i0) : kRowNT;
    R.out = (int64_t)R.s * A.n + R.i;
    return R;
}

// Slots c0 .. c0 + 31 of the tile's rows into tile[row * kRowLD + slot - c0] by loads that run along the rows (VEC: 16
// bytes a lane, a wavefront reads whole 128-byte pieces of eight rows; else 4 bytes a lane, two rows).  Rows without an
// EV are never read: zeros for them and past T.
template <bool VEC>
__device__ __forceinline__ void rows_stage(float *tile, const int *act, const RowsIn &A, const RowStart &R, int c0) {
    const int tid = threadIdx.x, T = A.T;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < kRowTC / 4; ++k) {    // piece e of the tile's chunk: row e / 8, slots c0 + 4 (e % 8) ..
            const int e = k * kRowNT + tid, r = e / (kRowTC / 4), t = 4 * (e % (kRowTC / 4));
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < R.rows_here && act[r]) {
                const float *src = R.base + (int64_t)r * A.stride_i + c0 + t;
                if (c0 + t + 3 < T) x = *reinterpret_cast<const float4 *>(src);
                else {
                    if (c0 + t < T) x.x = src[0];
                    if (c0 + t + 1 < T) x.y = src[1];
                    if (c0 + t + 2 < T) x.z = src[2];
                }
            }
            float *dst = tile + r * kRowLD + t;
            dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
        }
    } else {
#pragma unroll 8
        for (int k = 0; k < kRowTC; ++k) {        // element e of the tile's chunk: row e / 32, slot c0 + e % 32
            const int e = k * kRowNT + tid, r = e / kRowTC, t = e % kRowTC;
            float x = 0.f;
            if (r < R.rows_here && act[r] && c0 + t < T) x = R.base[(int64_t)r * A.stride_i + c0 + t];
            tile[r * kRowLD + t] = x;
        }
    }
}

// The wavefront's rows for which cond[c] holds, into cell[c]: cell is the wavefront's counters of the slot.
template <int USED>
__device__ __forceinline__ void rows_slot_ballot(int *cell, const bool (&cond)[USED]) {
    static_assert(USED <= kRowSlotC, "");
    unsigned long long b[USED];
    for (int c = 0; c < USED; ++c) b[c] = __ballot(cond[c]);
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < USED; ++c) cell[c] = __popcll(b[c]);
}

// The chunk's tc slots: the wavefronts' counts added, one global atomic per (slot, counter < USED) that is not zero.
// (threads 128 ..: the first threads may have a column of partial sums to write)
template <int USED>
__device__ __forceinline__ void rows_slot_flush(const int (*wcnt)[kRowTC][kRowSlotC], int32_t *slotc, uint32_t s, int T,
                                                int c0, int tc) {
    const int tid = threadIdx.x;
    if (tid >= 128 && tid - 128 < tc * kRowSlotC) {
        const int j = (tid - 128) / kRowSlotC, c = (tid - 128) % kRowSlotC;
        if (c < USED) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < kRowNT / 64; ++w) v += wcnt[w][j][c];
            if (v) atomicAdd(slotc + ((int64_t)s * T + c0 + j) * kRowSlotC + c, v);
        }
    }
}

// The workgroup's day counters and its PLANES histograms of T + 1 bins each, zeroed (visible after the next barrier).
template <int PLANES>
__device__ __forceinline__ void rows_day_clear(int *dcnt, int *lhist, bool hist, int T) {
    const int tid = threadIdx.x;
    if (tid < kRowDayC) dcnt[tid] = 0;
    if (hist)
        for (int k = tid; k < PLANES * (T + 1); k += kRowNT) lhist[k] = 0;
}

// The wavefront's rows for which cond[c] holds, added to dcnt[c].
__device__ __forceinline__ void rows_day_count(int *dcnt, const bool (&cond)[5]) {
    unsigned long long b[5];
    for (int c = 0; c < 5; ++c) b[c] = __ballot(cond[c]);
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 5; ++c)
            if (b[c]) atomicAdd(&dcnt[c], __popcll(b[c]));
}

// After a barrier behind the last LDS add: one global atomic per day counter and per histogram bin that is not zero.
template <int PLANES>
__device__ __forceinline__ void rows_day_flush(const int *dcnt, const int *lhist, int32_t *dayc, int32_t *hist, uint32_t s,
                                               int T) {
    const int tid = threadIdx.x;
    if (tid >= 64 && tid < 64 + kRowDayC && dcnt[tid - 64]) atomicAdd(dayc + (int64_t)s * kRowDayC + (tid - 64), dcnt[tid - 64]);
    if (hist)
        for (int k = tid; k < PLANES * (T + 1); k += kRowNT)
            if (lhist[k]) atomicAdd(hist + (int64_t)s * PLANES * (T + 1) + k, lhist[k]);
}

// What a fold and a day kernel read and write.
template <class SlotRec, class DayRec>
struct RowsFoldArgs {
    RowsScratch w;
    SlotRec *slot_rec;
    DayRec *day_rec;
    uint32_t nwg;
    int32_t T;
};

// A fold workgroup owns 32 columns of one scenario (grid.y) of ppart, double[S][nwg][C]: thread (segment, column) adds
// the segment's workgroups -- a contiguous 32nd of them -- in order, consecutive lanes on consecutive columns, then one
// thread a column adds the 32 segments in order: a fixed order, 32 chains instead of one.  A thread carries NV columns,
// `apart` apart; `inside`: its first column exists.  True for the one thread a column that then holds the sums in acc;
// the others are done.
template <int NV>
__device__ __forceinline__ bool rows_fold(double (*part)[kRowFoldSeg][kRowFoldCols + 1], const double *ppart, uint32_t nwg,
                                          int64_t C, int apart, bool inside, double (&acc)[NV]) {
    const int tid = threadIdx.x, lane = tid % kRowFoldCols, seg = tid / kRowFoldCols;
    const uint32_t len = (nwg + kRowFoldSeg - 1) / kRowFoldSeg;
    const uint32_t w0 = (uint32_t)seg * len, w1 = w0 + len < nwg ? w0 + len : nwg;
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    if (inside) {
        const double *pp = ppart + (int64_t)blockIdx.y * nwg * C + (int)blockIdx.x * kRowFoldCols + lane;
        for (uint32_t w = w0; w < w1; ++w)
            for (int v = 0; v < NV; ++v) acc[v] = acc[v] + pp[(int64_t)w * C + v * apart];
    }
    for (int v = 0; v < NV; ++v) part[v][seg][lane] = acc[v];
    __syncthreads();
    if (seg != 0 || !inside) return false;
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
#pragma unroll 8
    for (int q = 0; q < kRowFoldSeg; ++q)
        for (int v = 0; v < NV; ++v) acc[v] = acc[v] + part[v][q][lane];
    return true;
}

// ---- the host side ------------------------------------------------------------------------------------------------------

inline bool rows_sizes_ok(int32_t S, int64_t n, int32_t T) {
    return study_sizes_ok(S, n) && T >= 1 && T <= REVS_MAX_T;
}
inline int64_t rows_int_bytes(int32_t S, int32_t T) {            // the counters in front of the scratch
    return ((int64_t)S * T * kRowSlotC + (int64_t)S * kRowDayC) * (int64_t)sizeof(int32_t);
}
inline int64_t rows_scratch_bytes(int32_t S, int64_t n, int32_t T, int64_t C) {
    if (!rows_sizes_ok(S, n, T)) return 0;
    const int64_t nwg = (n + kRowNT - 1) / kRowNT;
    const int64_t bytes = rows_int_bytes(S, T) + (int64_t)S * (nwg + 1) * C * (int64_t)sizeof(double);
    return (bytes + 15) / 16 * 16;
}
inline RowsScratch rows_scratch(void *scratch, int32_t S, int32_t T, int64_t C) {
    RowsScratch W;
    W.slotc = (int32_t *)scratch; W.dayc = W.slotc + (int64_t)S * T * kRowSlotC;
    W.folded = (double *)((char *)scratch + rows_int_bytes(S, T));
    W.ppart = W.folded + (int64_t)S * C;
    return W;
}

// The checks the reports' entry points share, and behind them the rows kernel's input.  any_output: one output pointer at
// least is not NULL.
inline int rows_args(const char *who, int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                     const revs_home_t *homes, double on_frac, double short_tol, const void *scratch, bool any_output,
                     RowsIn *in) {
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(rows_sizes_ok(S, n, T), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(p, "%s: null pointer argument p", who);
    REVS_REQUIRE(homes, "%s: null pointer argument homes", who);
    REVS_REQUIRE(rows_inner_i(S, n, T, stride_s, stride_i) >= 0, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    REVS_REQUIRE(on_frac >= 0.0, "%s: on_frac=%g is negative or a NaN", who, on_frac);
    REVS_REQUIRE(short_tol >= 0.0, "%s: short_tol=%g is negative or a NaN", who, short_tol);
    REVS_REQUIRE(scratch, "%s: null pointer argument scratch", who);
    REVS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    REVS_REQUIRE(any_output, "%s: every output is NULL", who);
    in->p = p; in->homes = homes; in->stride_s = stride_s; in->stride_i = stride_i;
    in->n = (uint32_t)n; in->S = (uint32_t)S; in->nwg = (uint32_t)((n + kRowNT - 1) / kRowNT); in->T = T;
    return REVS_OK;
}

// rows_stage<true> may be used: every row begins on a 16-byte boundary.
inline bool rows_vec_ok(const RowsIn &A) {
    return ((uintptr_t)A.p & 15) == 0 && A.stride_s % 4 == 0 && A.stride_i % 4 == 0;
}

// The buffers that are not NULL cleared on the stream, in order (the counters of the scratch, hist, ...).
struct RowsClear { void *ptr; size_t bytes; };
template <int N>
inline int rows_clear(const char *who, hipStream_t st, const RowsClear (&bufs)[N]) {
    for (const RowsClear &b : bufs)
        if (b.ptr && hipMemsetAsync(b.ptr, 0, b.bytes, st) != hipSuccess) {
            revs::set_error("%s: clearing the counters failed", who);
            return REVS_ELAUNCH;
        }
    return REVS_OK;
}

// Where slot or day records are asked for: the fold of C columns a scenario, then the day kernel for the day records.
template <class F>
inline int rows_fold_launch(const char *who, hipStream_t st, void (*fold)(F), void (*day)(F), const F &args, int C, int32_t S) {
    if (!args.slot_rec && !args.day_rec) return REVS_OK;
    hipLaunchKernelGGL(fold, dim3((unsigned)((C + kRowFoldCols - 1) / kRowFoldCols), (unsigned)S),
                       dim3(kRowFoldSeg * kRowFoldCols), 0, st, args);
    REVS_CHECK_LAUNCH(who);
    if (args.day_rec) {
        hipLaunchKernelGGL(day, dim3((unsigned)S), dim3(256), 0, st, args);
        REVS_CHECK_LAUNCH(who);
    }
    return REVS_OK;
}

}  // namespace revs
