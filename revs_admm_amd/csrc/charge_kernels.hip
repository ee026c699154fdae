// The charging report (include/revs_admm_ops.h, "charging report"): what the chargers do, per EV
// and per slot, from the charger power where it lies.
//
//   charge_rows_kernel<VEC>  rows_pass.h's row pass.  Thread r steps row r's state machine through the staged chunk in
//                            slot order (one accumulator each for energy and cost: the bits of the sequential loop), the
//                            wavefronts ballot the slot's four conditions, and the chunk ends with one double per slot
//                            into the workgroup's row of partial sums: the tile's column sums, 32 rows a thread in row
//                            order, then the eight groups in order.
//   charge_fold_kernel       the partial sums are T + 1 columns a workgroup (the slots, then the cost), folded by
//                            rows_pass.h's chain; the thread that holds a slot's sum writes the slot record.
//   charge_day_kernel        one workgroup per scenario scans the folded slots for the day record.
#include "common.h"
#include "rows_pass.h"

#include <math.h>

// every product and sum is rounded on its own (bill_kernels.hip's note on the pragma holds here too)
#pragma clang fp contract(off)

namespace revs {

// slot counters: plugged, on, full, starts; day counters: n_ev, under, never, interrupted, outside
struct ChargeArgs {
    RowsIn in;
    const double *tariff;
    revs_charge_row_t *row_rec;
    int32_t *hist;
    double *val_out;
    uint8_t *keep_out;
    RowsScratch w;                                // T + 1 columns: the slots' power, then the cost
    double on_frac, short_tol;
};

template <bool VEC>
__global__ __launch_bounds__(kRowNT) void charge_rows_kernel(ChargeArgs A) {
    __shared__ float tile[kRowNT * kRowLD];
    __shared__ int act[kRowNT];                   // the row is there and has an EV
    __shared__ int wcnt[kRowNT / 64][kRowTC][kRowSlotC];
    __shared__ double colpart[kRowNT / 32][kRowTC];
    __shared__ double rowcost[kRowNT];
    __shared__ double cost8[kRowNT / 32];
    __shared__ int dcnt[kRowDayC];
    __shared__ int lhist[3 * (REVS_MAX_T + 1)];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int T = A.in.T;
    const RowStart R = rows_start(A.in, act);
    const revs_home_t &h = R.h;
    const bool ev = R.ev;
    const int ws = R.ws, we = R.we;
    rows_day_clear<3>(dcnt, lhist, A.hist != nullptr, T);
    const double rating = (double)h.rating, thr = A.on_frac * rating;
    double *ppart = A.w.ppart + ((int64_t)R.s * A.in.nwg + blockIdx.x) * (T + 1);   // the workgroup's row

    double energy = 0.0, cost = A.tariff ? 0.0 : __builtin_nan("");
    int n_on = 0, n_full = 0, first_on = -1, last_on = -1, sessions = 0, n_outside = 0;
    bool prev = false, bad = false;
    for (int c0 = 0; c0 < T; c0 += kRowTC) {
        __syncthreads();                          // (act is visible; the chunk before is read)
        rows_stage<VEC>(tile, act, A.in, R, c0);
        __syncthreads();
        const int tc = T - c0 < kRowTC ? T - c0 : kRowTC;
        const float *row = tile + tid * kRowLD;
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
            rows_slot_ballot(wcnt[wave][j], {plugged, on, full, start});
        }
        {   // the tile's column sums: rows 32 q .. 32 q + 31 of slot j in row order (rows without an EV hold zeros)
            const int j = tid & 31, q = tid >> 5;
            double acc = 0.0;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) acc = acc + (double)tile[(q * 32 + r) * kRowLD + j];
            colpart[q][j] = acc;
        }
        __syncthreads();
        if (tid < tc) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < kRowNT / 32; ++q) acc = acc + colpart[q][tid];
            ppart[c0 + tid] = acc;
        }
        rows_slot_flush<4>(wcnt, A.w.slotc, R.s, T, c0, tc);
    }

    // ---- the row's record
    const double soc = (double)h.initial + energy / (double)h.capacity;
    const double top = (double)h.initial > 0.9 ? (double)h.initial : 0.9;
    const bool under = ev && top - soc > A.short_tol;
    const int wait = first_on < 0 ? -1 : first_on - ws;
    const float soc_end = (float)soc;
    const int64_t out = R.out;
    if (R.there) {
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
            const int64_t plane = (int64_t)A.in.S * A.in.n;
            A.val_out[out] = keep ? energy : nan;
            A.val_out[plane + out] = keep ? cost : nan;
            A.val_out[2 * plane + out] = keep ? (double)soc_end : nan;
            A.val_out[3 * plane + out] = keep && first_on >= 0 ? (double)wait : nan;
        }
        if (A.keep_out) A.keep_out[out] = keep ? 1 : 0;
    }
    // ---- the workgroup's share of the day record and of the histograms
    rows_day_count(dcnt, {ev, under, ev && n_on == 0, ev && sessions > 1, ev && n_outside > 0});
    if (A.hist && ev) {
        atomicAdd(&lhist[n_on], 1);
        if (wait >= 0) atomicAdd(&lhist[(T + 1) + wait], 1);
        atomicAdd(&lhist[2 * (T + 1) + sessions], 1);
    }
    rowcost[tid] = ev ? cost : 0.0;
    __syncthreads();
    if (tid < kRowNT / 32) {
        double acc = 0.0;
        for (int r = 0; r < 32; ++r) acc = acc + rowcost[tid * 32 + r];
        cost8[tid] = acc;
    }
    rows_day_flush<3>(dcnt, lhist, A.w.dayc, A.hist, R.s, T);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < kRowNT / 32; ++q) acc = acc + cost8[q];
        ppart[T] = acc;
    }
}

using ChargeFoldArgs = RowsFoldArgs<revs_charge_slot_t, revs_charge_day_t>;   // folded: double[S][T + 1]

__global__ __launch_bounds__(kRowFoldSeg * kRowFoldCols) void charge_fold_kernel(ChargeFoldArgs A) {
    __shared__ double part[1][kRowFoldSeg][kRowFoldCols + 1];
    const int T = A.T, C = T + 1, col = (int)blockIdx.x * kRowFoldCols + (int)threadIdx.x % kRowFoldCols;
    const int64_t s = blockIdx.y;
    double acc[1];
    if (!rows_fold<1>(part, A.w.ppart, A.nwg, C, 0, col < C, acc)) return;
    A.w.folded[s * C + col] = acc[0];
    if (col < T && A.slot_rec) {
        const int32_t *c = A.w.slotc + (s * T + col) * kRowSlotC;
        revs_charge_slot_t r;
        r.n_ev = A.w.dayc[s * kRowDayC]; r.n_plugged = c[0]; r.n_on = c[1]; r.n_full = c[2]; r.n_starts = c[3]; r.reserved = 0;
        r.power = acc[0];
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
        power[tid] = A.w.folded[s * (T + 1) + tid];
        non[tid] = A.w.slotc[(s * T + tid) * kRowSlotC + 1];
    }
    __syncthreads();
    if (tid != 0) return;
    const int32_t *dc = A.w.dayc + s * kRowDayC;
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
    d.cost = A.w.folded[s * (T + 1) + T];
    d.peak_on = po; d.peak_on_slot = n_ev ? pos : -1; d.peak_power_slot = n_ev ? pks : -1;
    d.n_ev = n_ev; d.n_under = dc[1]; d.n_never = dc[2]; d.n_interrupted = dc[3]; d.n_outside = dc[4];
    A.day_rec[s] = d;
}

}  // namespace revs

using namespace revs;

extern "C" int32_t revs_charge_report_chunk(void) { return kRowTC; }

extern "C" int64_t revs_charge_report_scratch(int32_t S, int64_t n, int32_t T) {
    return rows_scratch_bytes(S, n, T, (int64_t)T + 1);
}

extern "C" int revs_charge_report(int32_t S, int64_t n, int32_t T, const float *p, int64_t stride_s, int64_t stride_i,
                                  const revs_home_t *homes, const double *tariff, double on_frac, double short_tol,
                                  revs_charge_row_t *row_rec, revs_charge_slot_t *slot_rec, revs_charge_day_t *day_rec,
                                  int32_t *hist, double *val_out, uint8_t *keep_out, void *scratch, void *stream) {
    static_assert(sizeof(revs_charge_row_t) == 64 && sizeof(revs_charge_slot_t) == 32 && sizeof(revs_charge_day_t) == 64, "");
    const char *who = "revs_charge_report";
    ChargeArgs A;
    if (int rc = rows_args(who, S, n, T, p, stride_s, stride_i, homes, on_frac, short_tol, scratch,
                           row_rec || slot_rec || day_rec || hist || val_out || keep_out, &A.in))
        return rc;

    hipStream_t st = (hipStream_t)stream;
    A.tariff = tariff; A.row_rec = row_rec; A.hist = hist; A.val_out = val_out; A.keep_out = keep_out;
    A.w = rows_scratch(scratch, S, T, T + 1);
    A.on_frac = on_frac; A.short_tol = short_tol;
    if (int rc = rows_clear(who, st, {{scratch, (size_t)rows_int_bytes(S, T)},
                                      {hist, (size_t)S * 3 * (T + 1) * sizeof(int32_t)}}))
        return rc;
    hipLaunchKernelGGL(rows_vec_ok(A.in) ? charge_rows_kernel<true> : charge_rows_kernel<false>, dim3(A.in.nwg, (unsigned)S),
                       dim3(kRowNT), 0, st, A);
    REVS_CHECK_LAUNCH(who);
    const ChargeFoldArgs F = {A.w, slot_rec, day_rec, A.in.nwg, T};
    return rows_fold_launch(who, st, charge_fold_kernel, charge_day_kernel, F, T + 1, S);
}
