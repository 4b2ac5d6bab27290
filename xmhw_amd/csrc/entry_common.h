// entry_common.h -- what the C entries of include/xmhw_amd.h share, whichever file they live in: capi.cpp (device,
// memory, plan, threshold and detect-chain entries) or the end of a stage's kernel file ("Entry layer").
// Declarations only: the definitions, and the process-wide caches behind them, are once in capi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace xmhw {
namespace entry {

// the calling thread's error text (xmhw_last_error) is set to msg; returns code
int fail(int code, const std::string& msg);
// a failed HIP call as XMHW_ERR_HIP, or XMHW_ERR_NOMEM where the device ran out of memory
int hip_fail(hipError_t e, const char* what);

// ---- the steps the stage entries share ----------------------------------------------------------
// Each is one call in the entry, in the entry's own order: which refusal wins when two apply, and which zero-size return
// comes before which NULL check, is part of the ABI (tests/test_host_entry_refusals.py).

// the status of an entry's last HIP call as the entry's own
int status_of(hipError_t e, const char* what);

// the one rule of a tuning knob whose values are 0 = automatic and any positive number: value < 0 is refused with
// XMHW_ERR_INVALID and the entry's message, anything else is stored
int set_knob(std::atomic<int>& knob, int32_t value, const char* message);

// An int32 host table kept on the device between calls, keyed by its content (capi.cpp, "per-call tables kept on the
// device between calls"), with what hangs on it: the chunk tables of the tiled exceedance kernel and the segment list
// of cooccur_accumulate.
struct ChunkTables {
    int32_t *tile_begin = nullptr, *t0 = nullptr, *i0 = nullptr, *n = nullptr;
    int32_t ntiles = 0;
    int64_t nchunks = 0;
};
struct RowsEntry {
    std::vector<int32_t> host;
    int device = 0;
    int32_t* d_rows = nullptr;
    std::map<std::pair<int64_t, int>, ChunkTables> chunks;      // (D, tile) -> tables
    void* d_segs = nullptr;                                     // class labels: the per-word segment list (cooccur_segments)
    int32_t *seg_off = nullptr, *seg_class = nullptr;
    uint64_t* seg_mask = nullptr;
    uint64_t stamp = 0;
    ~RowsEntry();
};
// The caller HOLDS the reference until its launches are queued: an entry another thread evicts meanwhile is destroyed
// (hipFree, which waits for the device) only when the last holder lets go of it.
using RowsRef = std::shared_ptr<RowsEntry>;

// an int32 host table on the device; the caller holds *table until its launches are queued
int upload_table(const int32_t* host, int64_t n, const char* what, RowsRef* table);

// The class labels as the segment list of the cooccur_accumulate kernel, built and uploaded once per label table (it hangs
// on the table's entry of the cache): seg_off[W + 1], then per segment -- a run of one non-negative class inside one
// 64-step word -- its class and the mask of its bits.
hipError_t cooccur_segments(const RowsRef& classes, int64_t Tn);

// scratch memory per (device, stream): grows on demand (the only synchronising moment), never shrinks.  A caller
// keeps the ScratchRef for the length of its call -- scratch->get() is its buffer: a buffer that another thread on the
// same stream outgrows meanwhile is freed only when its last holder is done.
using ScratchRef = std::shared_ptr<void>;
// `bytes` of this stream's scratch buffer; the caller holds *scratch until its launches are queued
int claim_scratch(hipStream_t st, size_t bytes, ScratchRef* scratch);

// the first step whose label lies outside [lo, hi), or n
int64_t first_outside(const int32_t* labels, int64_t n, int64_t lo, int64_t hi);
int check_labels(const int32_t* labels, int64_t n, int64_t lo, int64_t hi, const char* message);
constexpr const char* kRowsOutside = "row_of_t outside [0, D)";
constexpr const char* kClassesOutside = "class_of_t outside [-1, K)";

// the event-day bitmap of this call in this stream's scratch buffer: (T + 63) / 64 words per cell, leading dimension C
int event_day_bitmap(const uint64_t* bits, int64_t Tn, int64_t C, int64_t ldb, int32_t min_duration, int32_t join_gaps,
                     int32_t max_gap, hipStream_t st, ScratchRef* scratch, const uint64_t** inev);

}  // namespace entry
}  // namespace xmhw
