// The charging report (include/revs_admm_ops.h, "charging report"): what the chargers do, per EV
// and per slot, from the charger power where it lies.
//
//   charge_rows_kernel<VEC>  A workgroup owns 256 rows of ONE scenario (grid.y) and walks the slots in chunks of 32: the
//                            chunk of every EV row is staged in LDS by loads that run along the rows (VEC: 16 bytes a
//                            lane, a wavefront reads whole 128-byte pieces of eight rows; else 4 bytes a lane, two rows),
//                            rows without an EV are never read.  The LDS row stride is 33 words: thread r reads word
//                            33 r + t, which spreads a half wavefront over all banks, and the column sums read
//                            33 r + t with t along the lanes: consecutive banks.  Thread r then steps row r's state
//                            machine through the chunk in slot order (one accumulator each for energy and cost: the bits
//                            of the sequential loop), the wavefronts ballot the slot's four conditions into LDS counters,
//                            and the chunk ends with one global integer atomic per (slot, counter) that is not zero and
//                            one double per slot into the workgroup's row of partial sums (32 rows a thread in row
//                            order, then the eight groups in order).
//   charge_fold_kernel       the partial sums are T + 1 columns a workgroup (the slots, then the cost).  A fold workgroup
//                            owns 32 columns of one scenario: thread (segment, column) adds the segment's workgroups --
//                            a contiguous 32nd of them -- in order, consecutive lanes on consecutive columns, then one
//                            thread a column adds the 32 segments in order: a fixed order, 32 chains instead of one.
//   charge_day_kernel        one workgroup per scenario scans the folded slots for the day record.
#include "common.h"

#include <math.h>

// every product and sum is rounded on its own (bill_kernels.hip's note on the pragma holds here too)
#pragma clang fp contract(off)

namespace revs {

constexpr int kChgNT = 256;                       // rows of a tile: one thread each
constexpr int kChgTC = 32;                        // slots of a chunk: 128 bytes of a row
constexpr int kChgLD = kChgTC + 1;
constexpr int kChgSlotC = 4;                      // slot counters: plugged, on, full, starts
constexpr int kChgDayC = 8;                       // day counters: n_ev, under, never, interrupted, outside (8: 32 bytes)

struct ChargeArgs {
    const float *p;
    const revs_home_t *homes;
    const double *tariff;
    revs_charge_row_t *row_rec;
    int32_t *hist;
    double *val_out;
    uint8_t *keep_out;
    int32_t *slotc;                               // scratch int32[S][T][kChgSlotC]
    int32_t *dayc;                                // scratch int32[S][kChgDayC]
    double *ppart;                                // scratch double[S][nwg][T + 1]: the slots' power, then the cost
    int64_t stride_s, stride_i;
    double on_frac, short_tol;
    uint32_t n, S, nwg;
    int32_t T;
};

template <bool VEC>
__global__ __launch_bounds__(kChgNT) void charge_rows_kernel(ChargeArgs A) {
    __shared__ float tile[kChgNT * kChgLD];
    __shared__ int act[kChgNT];                   // the row is there and has an EV
    __shared__ int wcnt[kChgNT / 64][kChgTC][kChgSlotC];
    __shared__ double colpart[kChgNT / 32][kChgTC];
    __shared__ double rowcost[kChgNT];
    __shared__ double cost8[kChgNT / 32];
    __shared__ int dcnt[kChgDayC];
    __shared__ int lhist[3 * (REVS_MAX_T + 1)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = A.T;
    const uint32_t s = blockIdx.y, i0 = (uint32_t)blockIdx.x * kChgNT, i = i0 + (uint32_t)tid;
    const bool there = i < A.n;
    revs_home_t h;
    h.ev = 0; h.start = h.end = h.nmin = h.nmax = 0; h.rating = h.capacity = h.initial = 0.0f;
    if (there) h = A.homes[(int64_t)i * A.S + s];
    const bool ev = there && h.ev != 0;
    act[tid] = ev ? 1 : 0;
    if (tid < kChgDayC) dcnt[tid] = 0;
    if (A.hist)
        for (int k = tid; k < 3 * (T + 1); k += kChgNT) lhist[k] = 0;
    const int ws = h.start < 0 ? 0 : h.start > T ? T : h.start, we = h.end < 0 ? 0 : h.end > T ? T : h.end;
    const double rating = (double)h.rating, thr = A.on_frac * rating;
    const float *base = A.p + (int64_t)s * A.stride_s + (int64_t)i0 * A.stride_i;
    const int rows_here = A.n - i0 < (uint32_t)kChgNT ? (int)(A.n - i0) : kChgNT;

    double energy = 0.0, cost = A.tariff ? 0.0 : __builtin_nan("");
    int n_on = 0, n_full = 0, first_on = -1, last_on = -1, sessions = 0, n_outside = 0;
    bool prev = false, bad = false;
    for (int c0 = 0; c0 < T; c0 += kChgTC) {
        __syncthreads();                          // (act is visible; the chunk before is read)
        if (VEC) {
#pragma unroll
            for (int k = 0; k < kChgTC / 4; ++k) {   // piece e of the tile's chunk: row e / 8, slots c0 + 4 (e % 8) ..
                const int e = k * kChgNT + tid, r = e / (kChgTC / 4), t = 4 * (e % (kChgTC / 4));
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < rows_here && act[r]) {
                    const float *src = base + (int64_t)r * A.stride_i + c0 + t;
                    if (c0 + t + 3 < T) x = *reinterpret_cast<const float4 *>(src);
                    else {
                        if (c0 + t < T) x.x = src[0];
                        if (c0 + t + 1 < T) x.y = src[1];
                        if (c0 + t + 2 < T) x.z = src[2];
                    }
                }
                float *dst = tile + r * kChgLD + t;
                dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
            }
        } else {
#pragma unroll 8
            for (int k = 0; k < kChgTC; ++k) {    // element e of the tile's chunk: row e / 32, slot c0 + e % 32
                const int e = k * kChgNT + tid, r = e / kChgTC, t = e % kChgTC;
                float x = 0.f;
                if (r < rows_here && act[r] && c0 + t < T) x = base[(int64_t)r * A.stride_i + c0 + t];
                tile[r * kChgLD + t] = x;
            }
        }
        __syncthreads();
        const int tc = T - c0 < kChgTC ? T - c0 : kChgTC;
        const float *row = tile + tid * kChgLD;
        for (int j = 0; j < tc; ++j) {
            const int t = c0 + j;
            const double d = (double)row[j];
            energy = energy + d;
            if (A.tariff) cost = cost + A.tariff[t] * d;
            bad = bad || !(d - d == 0.0);
            const bool on = ev && d > thr, full = on && d >= rating, start = on && !prev;
            const bool plugged = ev && ws <= t && t < we;
            if (on) {
                ++n_on;
                if (first_on < 0) first_on = t;
                last_on = t;
                if (!plugged) ++n_outside;
            }
            n_full += full ? 1 : 0;
            sessions += start ? 1 : 0;
            prev = on;
            const unsigned long long b0 = __ballot(plugged), b1 = __ballot(on), b2 = __ballot(full), b3 = __ballot(start);
            if (lane == 0) {
                wcnt[wave][j][0] = __popcll(b0); wcnt[wave][j][1] = __popcll(b1);
                wcnt[wave][j][2] = __popcll(b2); wcnt[wave][j][3] = __popcll(b3);
            }
        }
        {   // the tile's column sums: rows 32 q .. 32 q + 31 of slot j in row order (rows without an EV hold zeros)
            const int j = tid & 31, q = tid >> 5;
            double acc = 0.0;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) acc = acc + (double)tile[(q * 32 + r) * kChgLD + j];
            colpart[q][j] = acc;
        }
        __syncthreads();
        if (tid < tc) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < kChgNT / 32; ++q) acc = acc + colpart[q][tid];
            A.ppart[((int64_t)s * A.nwg + blockIdx.x) * (T + 1) + c0 + tid] = acc;
        } else if (tid >= 128 && tid - 128 < tc * kChgSlotC) {
            const int j = (tid - 128) / kChgSlotC, c = (tid - 128) % kChgSlotC;
            int v = 0;
#pragma unroll
            for (int w = 0; w < kChgNT / 64; ++w) v += wcnt[w][j][c];
            if (v) atomicAdd(A.slotc + ((int64_t)s * T + c0 + j) * kChgSlotC + c, v);
        }
    }

    // ---- the row's record
    const double soc = (double)h.initial + energy / (double)h.capacity;
    const double top = (double)h.initial > 0.9 ? (double)h.initial : 0.9;
    const bool under = ev && top - soc > A.short_tol;
    const int wait = first_on < 0 ? -1 : first_on - ws;
    const float soc_end = (float)soc;
    const int64_t out = (int64_t)s * A.n + i;
    if (there) {
        if (A.row_rec) {
            revs_charge_row_t r;
            r.energy = ev ? energy : 0.0; r.cost = ev ? cost : 0.0;
            r.soc_end = ev ? soc_end : 0.f; r.reserved0 = 0.f;
            r.n_on = n_on; r.n_full = n_full; r.first_on = first_on; r.last_on = last_on; r.sessions = sessions;
            r.wait = wait; r.n_outside = n_outside;
            r.flags = ev ? 1 | (under ? 2 : 0) | (bad ? 4 : 0) : 0;
            r.reserved[0] = r.reserved[1] = 0;
            A.row_rec[out] = r;
        }
        const bool keep = ev && !bad;
        if (A.val_out) {
            const double nan = __builtin_nan("");
            const int64_t plane = (int64_t)A.S * A.n;
            A.val_out[out] = keep ? energy : nan;
            A.val_out[plane + out] = keep ? cost : nan;
            A.val_out[2 * plane + out] = keep ? (double)soc_end : nan;
            A.val_out[3 * plane + out] = keep && first_on >= 0 ? (double)wait : nan;
        }
        if (A.keep_out) A.keep_out[out] = keep ? 1 : 0;
    }
    // ---- the workgroup's share of the day record and of the histograms
    {
        const unsigned long long b0 = __ballot(ev), b1 = __ballot(under), b2 = __ballot(ev && n_on == 0),
                                 b3 = __ballot(ev && sessions > 1), b4 = __ballot(ev && n_outside > 0);
        if (lane == 0) {
            if (b0) atomicAdd(&dcnt[0], __popcll(b0));
            if (b1) atomicAdd(&dcnt[1], __popcll(b1));
            if (b2) atomicAdd(&dcnt[2], __popcll(b2));
            if (b3) atomicAdd(&dcnt[3], __popcll(b3));
            if (b4) atomicAdd(&dcnt[4], __popcll(b4));
        }
    }
    if (A.hist && ev) {
        atomicAdd(&lhist[n_on], 1);
        if (wait >= 0) atomicAdd(&lhist[(T + 1) + wait], 1);
        atomicAdd(&lhist[2 * (T + 1) + sessions], 1);
    }
    rowcost[tid] = ev ? cost : 0.0;
    __syncthreads();
    if (tid < kChgNT / 32) {
        double acc = 0.0;
        for (int r = 0; r < 32; ++r) acc = acc + rowcost[tid * 32 + r];
        cost8[tid] = acc;
    }
    if (tid >= 64 && tid < 64 + kChgDayC && dcnt[tid - 64]) atomicAdd(A.dayc + (int64_t)s * kChgDayC + (tid - 64), dcnt[tid - 64]);
    if (A.hist)
        for (int k = tid; k < 3 * (T + 1); k += kChgNT)
            if (lhist[k]) atomicAdd(A.hist + (int64_t)s * 3 * (T + 1) + k, lhist[k]);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < kChgNT / 32; ++q) acc = acc + cost8[q];
        A.ppart[((int64_t)s * A.nwg + blockIdx.x) * (T + 1) + T] = acc;
    }
}

constexpr int kChgFoldSeg = 32;                   // chains a column's workgroups are folded in
constexpr int kChgFoldCols = 32;                  // columns of a fold workgroup

struct ChargeFoldArgs {
    const int32_t *slotc, *dayc;
    const double *ppart;
    double *folded;                               // scratch double[S][T + 1]
    revs_charge_slot_t *slot_rec;
    revs_charge_day_t *day_rec;
    uint32_t nwg;
    int32_t T;
};

__global__ __launch_bounds__(kChgFoldSeg * kChgFoldCols) void charge_fold_kernel(ChargeFoldArgs A) {
    __shared__ double part[kChgFoldSeg][kChgFoldCols + 1];
    const int tid = threadIdx.x, lane = tid % kChgFoldCols, seg = tid / kChgFoldCols;
    const int T = A.T, C = T + 1, col = (int)blockIdx.x * kChgFoldCols + lane;
    const int64_t s = blockIdx.y;
    const uint32_t len = (A.nwg + kChgFoldSeg - 1) / kChgFoldSeg;
    const uint32_t w0 = (uint32_t)seg * len, w1 = w0 + len < A.nwg ? w0 + len : A.nwg;
    double acc = 0.0;
    if (col < C) {
        const double *pp = A.ppart + s * A.nwg * C + col;
        for (uint32_t w = w0; w < w1; ++w) acc = acc + pp[(int64_t)w * C];
    }
    part[seg][lane] = acc;
    __syncthreads();
    if (seg != 0 || col >= C) return;
    acc = 0.0;
#pragma unroll 8
    for (int q = 0; q < kChgFoldSeg; ++q) acc = acc + part[q][lane];
    A.folded[s * C + col] = acc;
    if (col < T && A.slot_rec) {
        const int32_t *c = A.slotc + (s * T + col) * kChgSlotC;
        revs_charge_slot_t r;
        r.n_ev = A.dayc[s * kChgDayC]; r.n_plugged = c[0]; r.n_on = c[1]; r.n_full = c[2]; r.n_starts = c[3]; r.reserved = 0;
        r.power = acc;
        A.slot_rec[s * T + col] = r;
    }
}

__global__ __launch_bounds__(256) void charge_day_kernel(ChargeFoldArgs A) {
    static_assert(REVS_MAX_T <= 256, "a thread per slot");
    __shared__ double power[REVS_MAX_T];
    __shared__ int non[REVS_MAX_T];
    const int tid = threadIdx.x, T = A.T;
    const int64_t s = blockIdx.x;
    if (tid < T) {
        power[tid] = A.folded[s * (T + 1) + tid];
        non[tid] = A.slotc[(s * T + tid) * kChgSlotC + 1];
    }
    __syncthreads();
    if (tid != 0) return;
    const int32_t *dc = A.dayc + s * kChgDayC;
    const int n_ev = dc[0];
    revs_charge_day_t d;
    double pk = power[0], en = 0.0;
    int pks = 0, po = non[0], pos = 0;
    for (int t = 0; t < T; ++t) {
        en = en + power[t];
        if (power[t] > pk) { pk = power[t]; pks = t; }
        if (non[t] > po) { po = non[t]; pos = t; }
    }
    d.peak_power = pk; d.energy = en;
    d.coincidence = n_ev ? (double)po / (double)n_ev : __builtin_nan("");
    d.cost = A.folded[s * (T + 1) + T];
    d.peak_on = po; d.peak_on_slot = n_ev ? pos : -1; d.peak_power_slot = n_ev ? pks : -1;
    d.n_ev = n_ev; d.n_under = dc[1]; d.n_never = dc[2]; d.n_interrupted = dc[3]; d.n_outside = dc[4];
    A.day_rec[s] = d;
}

}  // namespace revs

using namespace revs;

static bool charge_sizes_ok(int32_t S, int64_t n, int32_t T) {
    return study_sizes_ok(S, n) && T >= 1 && T <= REVS_MAX_T;
}
static int64_t charge_int_bytes(int32_t S, int32_t T) {         // the counters in front of the scratch, a multiple of 16
    return ((int64_t)S * T * kChgSlotC + (int64_t)S * kChgDayC) * (int64_t)sizeof(int32_t);
}

extern "C" int32_t revs_charge_report_chunk(void) { return kChgTC; }

extern "C" int64_t revs_charge_report_scratch(int32_t S, int64_t n, int32_t T) {
    if (!charge_sizes_ok(S, n, T)) return 0;
    const int64_t nwg = (n + kChgNT - 1) / kChgNT;
    const int64_t bytes = charge_int_bytes(S, T) + (int64_t)S * (nwg + 1) * ((int64_t)T + 1) * (int64_t)sizeof(double);
    return (bytes + 15) / 16 * 16;
}

extern "C" int revs_charge_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                                  const revs_home_t *homes, const double *tariff, double on_frac, double short_tol,
                                  revs_charge_row_t *row_rec, revs_charge_slot_t *slot_rec, revs_charge_day_t *day_rec,
                                  int32_t *hist, double *val_out, uint8_t *keep_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_charge_row_t) == 64 && sizeof(revs_charge_slot_t) == 32 && sizeof(revs_charge_day_t) == 64, "");
    static_assert(sizeof(revs_home_t) == 32, "");
    const char *who = "revs_charge_report";
    REVS_REQUIRE(S >= 1 && S <= REVS_STUDY_MAX_S, "%s: S=%d outside 1..%d", who, (int)S, REVS_STUDY_MAX_S);
    REVS_REQUIRE(T > 0 && T <= REVS_MAX_T, "%s: T=%d outside 1..%d", who, (int)T, REVS_MAX_T);
    REVS_REQUIRE(n >= 1, "%s: n=%lld < 1", who, (long long)n);
    REVS_REQUIRE(charge_sizes_ok(S, n, T), "%s: S*n rows, 2^31 or more (S=%d, n=%lld)", who, (int)S, (long long)n);
    REVS_REQUIRE(p, "%s: null pointer argument p", who);
    REVS_REQUIRE(homes, "%s: null pointer argument homes", who);
    REVS_REQUIRE(rows_inner_i(S, n, T, stride_s, stride_i) >= 0, "%s: rows overlap under stride_s=%lld, stride_i=%lld (S=%d, n=%lld, T=%d)", who,
                 (long long)stride_s, (long long)stride_i, (int)S, (long long)n, (int)T);
    REVS_REQUIRE(on_frac >= 0.0, "%s: on_frac=%g is negative or a NaN", who, on_frac);
    REVS_REQUIRE(short_tol >= 0.0, "%s: short_tol=%g is negative or a NaN", who, short_tol);
    REVS_REQUIRE(scratch, "%s: null pointer argument scratch", who);
    REVS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    REVS_REQUIRE(row_rec || slot_rec || day_rec || hist || val_out || keep_out, "%s: every output is NULL", who);

    hipStream_t st = (hipStream_t)stream;
    const uint32_t nwg = (uint32_t)((n + kChgNT - 1) / kChgNT);
    const int64_t ib = charge_int_bytes(S, T);
    ChargeArgs A;
    A.p = p; A.homes = homes; A.tariff = tariff; A.row_rec = row_rec; A.hist = hist; A.val_out = val_out;
    A.keep_out = keep_out;
    A.slotc = (int32_t *)scratch; A.dayc = A.slotc + (int64_t)S * T * kChgSlotC;
    double *folded = (double *)((char *)scratch + ib);
    A.ppart = folded + (int64_t)S * (T + 1);
    A.stride_s = stride_s; A.stride_i = stride_i; A.on_frac = on_frac; A.short_tol = short_tol;
    A.n = (uint32_t)n; A.S = (uint32_t)S; A.nwg = nwg; A.T = T;
    if (hipMemsetAsync(scratch, 0, (size_t)ib, st) != hipSuccess
        || (hist && hipMemsetAsync(hist, 0, (size_t)S * 3 * (T + 1) * sizeof(int32_t), st) != hipSuccess)) {
        revs::set_error("%s: clearing the counters failed", who);
        return REVS_ELAUNCH;
    }
    const bool vec = ((uintptr_t)p & 15) == 0 && stride_s % 4 == 0 && stride_i % 4 == 0;
    const dim3 grid(nwg, (unsigned)S);
    if (vec) hipLaunchKernelGGL(charge_rows_kernel<true>, grid, dim3(kChgNT), 0, st, A);
    else hipLaunchKernelGGL(charge_rows_kernel<false>, grid, dim3(kChgNT), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    if (slot_rec || day_rec) {
        ChargeFoldArgs F;
        F.slotc = A.slotc; F.dayc = A.dayc; F.ppart = A.ppart; F.folded = folded; F.slot_rec = slot_rec; F.day_rec = day_rec;
        F.nwg = nwg; F.T = T;
        hipLaunchKernelGGL(charge_fold_kernel, dim3((unsigned)((T + 1 + kChgFoldCols - 1) / kChgFoldCols), (unsigned)S),
                           dim3(kChgFoldSeg * kChgFoldCols), 0, st, F);
        REVS_CHECK_LAUNCH(who);
        if (day_rec) {
            hipLaunchKernelGGL(charge_day_kernel, dim3((unsigned)S), dim3(256), 0, st, F);
            REVS_CHECK_LAUNCH(who);
        }
    }
    return REVS_OK;
}
