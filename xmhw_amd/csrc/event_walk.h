// event_walk.h -- mhw_filter() + join_gaps() (xmhw/identify.py:415-479, 273-325) for ONE cell on its
// exceedance words (bits[w * ldb + c], 64 consecutive steps per word: kernels_events.hip).  Shared by
// events_from_bits (the event table) and event_day_bits (the per-day in-event bitmap of mhw_coverage()):
// what happens to a finished event is the caller's `Sink`, called as sink(index, first, last) with the
// event's number within the cell, its label (= first labelled step) and its last step.
#pragma once
#include <stdint.h>

namespace xmhw {

// State of mhw_filter() + join_gaps() while walking the runs of one cell.
// A qualified run [s, e] (length test of identify.py:445-449 with the fillna(0) quirk: a run that
// begins at step 0 has p = 0, label 1, and loses its first step) either extends the pending
// event (gap to the previous qualified run <= maxGap) or closes it and opens a new one.
template <class Sink>
struct EventWalk {
    int64_t count = 0;
    bool have = false;            // a pending (not yet emitted) event
    int64_t first = 0, last = 0;  // its label (= first labelled step) and end step
    Sink sink;

    __device__ __forceinline__ void emit() {
        sink(count, first, last);
        ++count;
    }
    __device__ __forceinline__ void run(int64_t s, int64_t e, int32_t min_duration, int32_t join_gaps,
                                        int32_t max_gap) {
        const int64_t p = s > 0 ? s - 1 : 0;
        if (e - p < min_duration) return;
        const int64_t S = p + 1;
        if (have && join_gaps && S - last <= max_gap + 1) {
            last = e;
            return;
        }
        if (have) emit();
        have = true;
        first = S;
        last = e;
    }
    __device__ __forceinline__ void finish() {
        if (have) emit();
        have = false;
    }
};

// Walks the runs of ones of cell c and feeds them to ew (run() per qualified candidate, finish() at the end).
template <class Sink>
__device__ __forceinline__ void walk_exceed_bits(const uint64_t* __restrict__ bits, int64_t c, int64_t Tn, int64_t ldb,
                                                 int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                                                 EventWalk<Sink>& ew) {
    const int64_t W = (Tn + 63) / 64;
    bool in_run = false;
    int64_t s = 0;
    // Morphological opening by min_duration before the walk: runs shorter than min_duration can
    // never qualify (identify.py:445-449), and white-noise exceedances are mostly such runs.
    // eroded[t] = AND_{j<m} x[t+j] (needs the next word), opened[t] = OR_{j<m} eroded[t-j] (needs the
    // previous eroded word): every run of >= m ones survives unchanged, every shorter run vanishes.
    const int m = min_duration <= 64 ? min_duration : 1;
    constexpr int U = 4;
    uint64_t cur = bits[c];
    uint64_t er_prev = 0;
    for (int64_t w0 = 0; w0 < W; w0 += U) {
        uint64_t ws[U + 1];
        ws[0] = cur;
#pragma unroll
        for (int u = 1; u <= U; ++u) ws[u] = w0 + u < W ? bits[(w0 + u) * ldb + c] : 0;
        cur = ws[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (w0 + u >= W) break;
            const int64_t base = (w0 + u) * 64;
            uint64_t er = ws[u];
            for (int j = 1; j < m; ++j) er &= (ws[u] >> j) | (ws[u + 1] << (64 - j));
            uint64_t x = er;
            for (int j = 1; j < m; ++j) x |= (er << j) | (er_prev >> (64 - j));
            er_prev = er;
            int pos = 0;
            while (pos < 64) {
                const uint64_t rest = x >> pos;
                if (in_run) {
                    const uint64_t z = ~rest;                       // zeros of the remaining bits
                    if (z == 0) break;                              // pos == 0, all ones: continues
                    const int k = __builtin_ctzll(z);               // ones from pos on
                    if (pos + k >= 64) break;                       // the run continues into the next word
                    ew.run(s, base + pos + k - 1, min_duration, join_gaps, max_gap);
                    in_run = false;
                    pos += k;
                } else {
                    if (rest == 0) break;
                    const int k = __builtin_ctzll(rest);
                    s = base + pos + k;
                    in_run = true;
                    pos += k;
                }
            }
        }
    }
    if (in_run) ew.run(s, Tn - 1, min_duration, join_gaps, max_gap);   // bits beyond T-1 are zero
    ew.finish();
}

}  // namespace xmhw
