/*
 * xmhw_amd.h -- C ABI of the MI355X (gfx950) implementation of xmhw's
 * threshold() hot path.
 *
 * The reference (coecms/xmhw v0.9.3) is pure Python and has NO native
 * interface; this ABI is what a binding for the path would call.  Each entry
 * point names the reference code it replaces (paths relative to the reference
 * repository root).  Plain pointers and sizes only; no exceptions cross the
 * ABI: every function returns XMHW_OK or an error code and
 * xmhw_last_error() holds the message for the calling thread.
 *
 * Layout contract (the reference's land_check() output, identify.py:482-529):
 *   ts      [T][ld]  time-major, cell-minor ("cell" = stacked lat x lon);
 *                    element (t, c) at ts[t*ld + c], c < C <= ld
 *   doy     [T]      int32 label of every time step (add_doy(),
 *                    identify.py:28-79); HOST memory
 *   thresh  [D][ldo] float64, row i <-> i-th smallest distinct doy label
 *   seas    [D][ldo] float64
 * "dev" pointers are device (HBM) addresses owned by the caller.
 */
#ifndef XMHW_AMD_H
#define XMHW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMHW_OK 0
#define XMHW_ERR_INVALID 1     /* bad argument (the reference raises XmhwException) */
#define XMHW_ERR_HIP 2         /* HIP runtime error / no device                     */
#define XMHW_ERR_UNSUPPORTED 3 /* configuration outside every kernel's limits       */
#define XMHW_ERR_NOMEM 4
#define XMHW_ERR_COMM 5        /* RCCL could not be loaded / a collective failed     */

/* kernel selector for xmhw_plan_set_kernel() / reported by xmhw_plan_info() */
#define XMHW_KERNEL_AUTO 0
#define XMHW_KERNEL_RING 1     /* register-ring sliding-window kernel (fast path)   */
#define XMHW_KERNEL_GENERIC 2  /* one wave per (cell, doy), radix descent (any plan)*/

/* ---- library / device ------------------------------------------------- */
int xmhw_version(void);                 /* 1000*major + minor                     */
const char *xmhw_arch(void);            /* "gfx950"                               */
const char *xmhw_last_error(void);      /* message of the last failure (thread)   */
int xmhw_device_count(int *count);
int xmhw_set_device(int device);
int xmhw_get_device(int *device);
int xmhw_device_info(int device, char *name, int name_len, int *compute_units,
                     uint64_t *hbm_bytes);

/* ---- caller-owned device memory, streams, events ---------------------- */
int xmhw_malloc(void **dev_ptr, size_t bytes);
int xmhw_free(void *dev_ptr);
int xmhw_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, void *stream);
int xmhw_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, void *stream);
/* a block of columns of a row-major host array into a dense device array (hipMemcpy2D):
 * `height` rows of `width_bytes`, rows `spitch` bytes apart on the host, `dpitch` on the device */
int xmhw_memcpy2d_h2d(void *dev_dst, size_t dpitch, const void *host_src, size_t spitch,
                      size_t width_bytes, size_t height, void *stream);
/* the inverse for results: a dense device array into a block of columns of a row-major host array */
int xmhw_memcpy2d_d2h(void *host_dst, size_t dpitch, const void *dev_src, size_t spitch,
                      size_t width_bytes, size_t height, void *stream);
/* the same without the wait (one per rank of a gathered buffer, then ONE xmhw_stream_sync)   */
int xmhw_memcpy2d_d2h_async(void *dst, size_t dpitch, const void *src_dev, size_t spitch, size_t width,
                            size_t height, void *stream);
int xmhw_memset(void *dev_dst, int value, size_t bytes, void *stream);
/* ---- ingest: file bytes -> samples on the device ------------------------ *
 * The reference leaves reading and CF decoding to xarray (docs/gettingstarted.rst:30-33).  Here the
 * RAW bytes of a column slab cross PCIe (pinned staging: xmhw_host_alloc, asynchronous pitched
 * copy) and are decoded in HBM: byte order (netCDF classic is big-endian), CF packing
 * `raw * scale_factor + add_offset` in the arithmetic of the decoded type (float32 result: two
 * float32 roundings, as xarray computes it for float32 attributes), `_FillValue` -> NaN.
 * raw_itemsize 2 = int16, 4 = float32, 8 = float64; pairs: int16->float32/float64,
 * float32->float32, float64->float64.                                                          */
int xmhw_host_alloc(void **host_ptr, size_t bytes);        /* page-locked host memory */
int xmhw_host_free(void *host_ptr);
int xmhw_memcpy2d_h2d_async(void *dev_dst, size_t dpitch, const void *host_src, size_t spitch,
                            size_t width_bytes, size_t height, void *stream);
int xmhw_memcpy_h2d_async(void *dev_dst, const void *host_src, size_t bytes, void *stream);
int xmhw_memcpy_d2h_async(void *host_dst, const void *dev_src, size_t bytes, void *stream);
int xmhw_event_sync(void *event);                           /* block the host until the event has happened */
int xmhw_decode(const void *raw_dev, int raw_itemsize, int big_endian, int64_t rows, int64_t cols,
                int64_t ld_raw, void *out_dev, int out_itemsize, int64_t ld_out, int has_scale,
                double scale_factor, double add_offset, int has_fill, double fill_value, void *stream);
/* the inverse for float32 -> int16 codes (what writing a packed archive does: xarray's CF encoding): code =
 * rint((x - add_offset) / scale_factor) computed in float64 and clamped to [-32767, 32767]; NaN -> fill_code.  bench.py
 * and the tests make packed input for xmhw_clim_raw_i16 with it.                                              */
int xmhw_encode_i16(const float *in_dev, int64_t rows, int64_t cols, int64_t ld_in, int16_t *out_dev, int64_t ld_out,
                    double scale_factor, double add_offset, int32_t fill_code, void *stream);
/* File bytes -> a (page-locked) host buffer without mapping the file: `rows` strips of row_bytes bytes,
 * row_pitch apart in the file starting at file_offset, are read with pread() into a dense buffer.
 * Thread-safe; the ingest path calls it from many threads at once (copies out of an mmap() of the same
 * file queue up on the process's page-fault path instead).  Replaces the read half of
 * xr.open_dataset(...) (docs/gettingstarted.rst:30-33) for netCDF classic files.                   */
int xmhw_read_rows(int fd, int64_t file_offset, int64_t row_pitch, int64_t row_bytes, int64_t rows,
                   void *dst_host);
/* maxPadLength: `ts.interpolate_na(dim=tdim, max_gap=maxPadLength)` (xmhw/xmhw.py:159-160, :409-410;
 * xarray's linear interpolate_na with use_coordinate=True) on the device copy of a compacted series
 * (T, C), leading dimension ld, IN PLACE.  x_dev[T] = the numeric time coordinate (float64; for
 * datetime axes xarray uses nanoseconds since the first step).  A run of NaN strictly between valid
 * samples at steps a < b is filled iff x[b] - x[a] <= max_gap, with numpy.interp's float64 arithmetic
 * rounded to the sample type; leading / trailing runs and all-NaN cells are left alone.           */
int xmhw_pad_gaps(void *ts_dev, int itemsize, int64_t T, int64_t C, int64_t ld, const double *x_dev,
                  double max_gap, void *stream);
int xmhw_stream_create(void **stream);
int xmhw_stream_destroy(void *stream);
int xmhw_stream_sync(void *stream);     /* NULL = default stream                  */
int xmhw_event_create(void **event);
int xmhw_stream_wait_event(void *stream, void *event);   /* later work on `stream` waits for `event` */
int xmhw_event_destroy(void *event);
int xmhw_event_record(void *event, void *stream);
int xmhw_event_elapsed_ms(void *start, void *stop, float *ms); /* syncs on stop  */

/* ---- plan: everything derived from the doy labels ---------------------- *
 * Replaces the per-cell window_roll() bookkeeping (identify.py:184-209: which
 * samples pool under which doy) and groupby("doy") (identify.py:233,263).
 * Built on the host from doy[T]; device tables are uploaded on first use.   */
typedef struct xmhw_plan xmhw_plan;

int xmhw_plan_create(const int32_t *doy_host, int64_t T, int32_t window_half_width,
                     xmhw_plan **plan);
int xmhw_plan_destroy(xmhw_plan *plan);
/* D = number of distinct doy labels, ntracks = runs of increasing doy ("years"),
 * kernel = XMHW_KERNEL_* that AUTO resolves to for float32 input             */
int xmhw_plan_info(const xmhw_plan *plan, int32_t *D, int32_t *ntracks,
                   int32_t *kernel, int32_t *nsteps, int32_t *step_min);
int xmhw_plan_doys(const xmhw_plan *plan, int32_t *doys_out /* [D] */);
int xmhw_plan_set_kernel(xmhw_plan *plan, int32_t kernel);  /* tests / fallback */
/* float64 input whose samples are all float32-representable (decoded int16 / float32 archives) is
 * run through the float32 ring kernel (same pools, same float64 interpolation and sums of the same
 * values; 2.7x the float64 kernel's rate).  The check happens on the device inside
 * xmhw_clim_raw_f64 (sparse probe, then on every sample the kernel loads; the float64 kernel is
 * queued behind and runs only if a sample failed), so the call stays asynchronous.  Enabled by
 * default; xmhw_plan_narrowed() reports (synchronously) whether the last float64 call of this
 * plan stayed on the float32 kernel.                                                         */
int xmhw_plan_set_narrowing(xmhw_plan *plan, int32_t enable);
/* measurement (bench.py): with timing on, every xmhw_clim_raw_f32 / xmhw_clim_raw_i16 call records a HIP event on its
 * stream right before and right after its MAIN kernel (the sorted-list kernel -- which since round 6 also recomputes the
 * cell-rows its select cannot settle -- or the ring kernel); xmhw_plan_kernel_ms returns the elapsed time of the call
 * `calls_back` calls ago (0 = the last one, up to 15), waiting for it to finish.
 * A plan is used from ONE stream at a time: the timing events and the lazily uploaded tables belong to the plan, not to
 * the call.  Two calls on the same plan may be in flight only if they were issued on the same stream.               */
int xmhw_plan_set_timing(xmhw_plan *plan, int32_t enable);
int xmhw_plan_kernel_ms(xmhw_plan *plan, int32_t calls_back, float *ms);
int xmhw_plan_narrowed(xmhw_plan *plan, int32_t *narrowed_out);
int xmhw_plan_set_chunks(xmhw_plan *plan, int32_t nchunks); /* 0 = auto         */
/* how many chunks of the doy axis a launch over C cells is cut into (the automatic choice or the forced one):
 * every workgroup walks D / nchunks rows with output + 2w warm-up rows (csrc/route.cpp: ring_chunks)    */
int xmhw_plan_chunks_in_use(const xmhw_plan *plan, int64_t C, int32_t *nchunks);
/* host copy of the ring kernel's step table for inspection:
 * table[nsteps][ntracks_padded] (see csrc/plan.h for the encoding)            */
int xmhw_plan_table(const xmhw_plan *plan, int32_t years_per_lane, uint32_t *table_out,
                    int32_t *ntracks_padded);
/* the sorted-list kernel on this plan: keys a cell keeps of every row-list (for 37..40 tracks 16: 14 ranks in LDS, two in
 * registers), LDS bytes of a wave (32 cells; handed out in 1,280-byte pieces: 20,480 = 8 waves per CU), and the `pieces`
 * a launch over C cells asks xmhw_plan_sorted_table for (the automatic choice or xmhw_plan_set_chunks)            */
int xmhw_plan_sorted_info(const xmhw_plan *plan, int64_t C, int32_t *keys_per_list, int32_t *lds_bytes_per_wave,
                          int32_t *pieces);
/* host copy of the sorted-list kernel's chunks and step table (XMHW_LAYOUT_SORTED; csrc/plan.h: sorted_plan) for
 * inspection: the row axis cut wherever the set of pooled tracks changes (doy 60, the ends of partial years), every
 * chunk with its own table rows -- what window_roll() + groupby("doy") pool (xmhw/identify.py:184-209, :233) restated
 * per chunk.  `pieces` = how many pieces the whole row axis is cut into at least (1: only the cuts the calendar asks
 * for).  Call with NULL outputs for the sizes: nchunks, nrows (table / flag rows), ntp (entries per row, track k at
 * index k); then chunks_out[nchunks][4] = {warm_start, begin, end, trow0}, table_out[nrows][ntp], flags_out[nrows]
 * (in calendar order; a launch runs them longest first).
 * XMHW_ERR_UNSUPPORTED if the kernel is not instantiated for this plan.                                          */
int xmhw_plan_sorted_table(const xmhw_plan *plan, int32_t pieces, int32_t *nchunks, int32_t *nrows, int32_t *ntp,
                           int32_t *chunks_out, uint32_t *table_out, uint32_t *flags_out);
/* how many chunks of a float32 launch over C cells the sorted-list kernel settles DIRECTLY instead of walking their
 * table rows: chunks of one output row whose pool holds at most 12 tracks (Feb 29 of a daily record: the leap years
 * alone) -- the cell's pool is read once, its 24 largest keys give both order statistics (csrc/kernels_sorted.hip:
 * direct_row).  Chunks, table rows and results are the same either way; 0 with XMHW_SORTED_ONEROW=0 in the environment
 * (process-wide, read once).  int16 launches walk every chunk.
 * XMHW_ERR_UNSUPPORTED if the kernel is not instantiated for this plan.                                          */
int xmhw_plan_sorted_direct(const xmhw_plan *plan, int64_t C, int32_t *count);

/* debug: ring-kernel pass counters {rows, 32-bit count passes, extractions, cold starts,
 * fast steps, 8-bit probes, code-ring rebuilds} per wave, then count passes summed over CELLS (what
 * each cell needed on its own); all summed since the last read; the third-generation kernel
 * (layouts 20..22) reports its band-path counters in slots 5..7 (csrc/kernels_ring3.hip) and
 * shader-clock ticks per section of its row loop in slots 8..15.
 * The counters live in counter twins of the ring kernels that the PRODUCT build does not contain
 * (make STATS=1 builds them: tools/); xmhw_debug_stats_available() tells, and without them every
 * counter reads 0.
 * enable != 0 allocates the counters.  xmhw_plan_debug_stats_n: `out` receives min(n, 16) values.
 * xmhw_plan_debug_stats (the round-1 entry point): out8 receives the first 8 values.          */
int xmhw_debug_stats_available(void);
int xmhw_plan_debug_stats_n(xmhw_plan *plan, int enable, uint64_t *out, int32_t n);
int xmhw_plan_debug_stats(xmhw_plan *plan, int enable, uint64_t *out8);

/* ---- which ring kernel and lane layout float32 input runs on ------------- *
 * Every layout returns bit-identical thresh; the choice is about speed only.
 * XMHW_LAYOUT_AUTO (the default): the third-generation kernel (xmhw_amd/csrc/kernels_ring3.hip:
 * per-cell histogram in LDS, band compaction, sort across the lanes of a cell) on 2 lanes per cell
 * for 9..24 tracks, on 4 lanes for 25..48, on 8 lanes for 49..88; the second-generation kernel
 * (kernels_ring2.hip) on 16 lanes per cell for 89..96 tracks; the round-1 kernel otherwise.
 * A layout may be forced wherever it is instantiated (RING3_8LANE: 9..88 tracks, RING3_4LANE: 9..48,
 * RING3_2LANE: 9..24, RING2_8LANE / RING2_4LANE: 9..48, RING2_16LANE: 49..96); a plan it is not
 * instantiated for falls back to the round-1 kernel (xmhw_plan_layout_in_use tells).
 * The environment variable XMHW_RING2 sets the default of new plans (the same numbers).        */
enum {
    XMHW_LAYOUT_AUTO = -2,
    XMHW_LAYOUT_RING1 = -1,          /* round-1 kernel (csrc/kernels_ring.hip): other windows, > 96 or < 9 tracks;
                                      * forced on 9..96 tracks at w = 5 it runs on its 32-lane entries, padded   */
    XMHW_LAYOUT_RING2_8LANE = 8,     /* second generation, lists merged into the cell's 8 nearest keys */
    XMHW_LAYOUT_RING2_4LANE = 10,    /* second generation, 4 lanes per cell, 7 merged keys */
    XMHW_LAYOUT_RING2_16LANE = 12,   /* second generation, 16 lanes per cell: 49..96 tracks */
    XMHW_LAYOUT_RING3_8LANE = 20,    /* third generation, 8 cells per wave */
    XMHW_LAYOUT_RING3_4LANE = 21,    /* third generation, 16 cells per wave: the headline layout (40 tracks) */
    XMHW_LAYOUT_RING3_2LANE = 22,    /* third generation, 32 cells per wave */
    XMHW_LAYOUT_SORTED = 40          /* rounds 5-6 (csrc/kernels_sorted.hip): sorted row-lists in LDS + a parallel
                                        merge-select, 32 cells per wave, every row of the plan (chunks with their own
                                        table rows: plan.h); a cell-row whose lists are too short is recomputed inside
                                        the kernel.  float32 (or int16 codes), w = 5, 9..48 tracks.  NOTE: 40 means
                                        "sorted for quantiles >= 0.85 or <= 0.15": a call with a quantile in between runs the same plan
                                        on its ring layout (xmhw_plan_layout_in_use cannot know the call's quantile).
                                        Needs a device whose LDS reads outside the allocation return 0 (gfx950; probed
                                        once per device, otherwise the ring layouts serve the plan) */
};
int xmhw_plan_set_layout(xmhw_plan *plan, int32_t layout);
/* the layout float32 input of this plan will run on (XMHW_LAYOUT_RING1 if the round-1 / generic kernel) */
int xmhw_plan_layout_in_use(const xmhw_plan *plan, int32_t *layout);
/* whether the current device may run the sorted-list kernel: its rank-major lists rely on LDS reads outside a workgroup's
 * allocation returning 0 (gfx950 does: tools/ubench_ldsoob.hip).  Probed on the device the first time it is asked for
 * (seven allocation sizes x 2,048 workgroups, a few microseconds) and remembered per device; *holds = 1 / 0.  Plans on a
 * device where it does not hold run on their ring layout whatever xmhw_plan_layout_in_use says (which needs no device). */
int xmhw_sorted_device_ok(int32_t *holds);
/* DEPRECATED names of the two entries above (rounds 2 and 3, when the numbers meant variants of the
 * second-generation kernel); also accepted: 1..7, 9, 11 = measured-and-rejected alternatives of round 2,
 * built with -DXMHW_RING2_EXPERIMENTS only; 30..32 = the round-4 key-store experiment
 * (csrc/kernels_ring4.hip, built with `make RING4=1` only; profiles/r4_store_experiment.txt)          */
int xmhw_plan_set_ring2(xmhw_plan *plan, int32_t variant);
int xmhw_plan_ring2_in_use(const xmhw_plan *plan, int32_t *variant);
/* genuinely float64 samples (those that do not narrow to float32): the layout of the 64-bit mode
 * (64-bit keys as a high word -- what the selection runs on -- and a low word) this plan will run on:
 * 21 / 20 = the third-generation kernel on 4 lanes per cell (13..20 tracks) / 8 lanes per cell (9..12 and
 * 21..48 tracks; XMHW_RING3_F64=0 turns both off, XMHW_RING3_F64_LANES=8 the 4-lane layout),
 * 8 = the second-generation kernel on 8 lanes per cell (only with XMHW_RING3_F64=0), 12 = on 16 lanes per cell
 * (other records up to 96 tracks), or -1 (generic kernel).  w = 5.                              */
int xmhw_plan_f64_mode(const xmhw_plan *plan, int32_t *variant);
/* the whole route of one xmhw_clim_raw_f32 (elem_bytes 4) / _f64 (8) call with quantile q over C cells: what the
 * entries above report, and what the call launches, come from this one answer.  Needs no device (like
 * xmhw_plan_layout_in_use it assumes one that may run the sorted-list kernel).  out receives XMHW_ROUTE_WORDS values:
 *   [0]  XMHW_OK, or XMHW_ERR_UNSUPPORTED: the call would be refused (no launches)
 *   [1]  the number of launches (at most 3), queued in this order
 *   [2 + 7 i ...], i < 3 (zeros past the last launch):
 *        family (XMHW_ROUTE_*), layout (XMHW_LAYOUT_*; RING1 for the round-1 and generic kernels), lanes per cell,
 *        tracks per lane, narrows (float64 samples read as float32 behind the probe; stops at the first lossy sample),
 *        gated (runs only if the narrowing launch before it gave up), counters (takes the debug pass counters)
 *   [23] chunks of the doy axis of the ring launches (xmhw_plan_chunks_in_use)
 *   [24] pieces of the sorted-list kernel (xmhw_plan_sorted_info; 0: not instantiated for this plan)              */
enum { XMHW_ROUTE_GENERIC = 0, XMHW_ROUTE_RING1 = 1, XMHW_ROUTE_RING2 = 2, XMHW_ROUTE_RING3 = 3, XMHW_ROUTE_RING4 = 4,
       XMHW_ROUTE_SORTED = 5 };
#define XMHW_ROUTE_WORDS 25
int xmhw_plan_route(const xmhw_plan *plan, int32_t elem_bytes, double q, int64_t C, int32_t *out, int32_t n);

/* ---- the hot path ------------------------------------------------------ *
 * xmhw_clim_raw_*: for every cell, the pooled linear-interpolated quantile
 * and the pooled mean per doy -- calculate_thresh()/calculate_seas() WITHOUT
 * the Feb-29 step (identify.py:233-235, :263) over window_roll()'s pools.
 * NaN samples are dropped from the pools (identify.py:208); an empty pool
 * gives NaN.  negate != 0 computes on -ts (coldSpells, xmhw.py:153-154).
 * q = pctile / 100.0 (identify.py:234).                                      */
int xmhw_clim_raw_f32(xmhw_plan *plan, const float *ts_dev, int64_t C, int64_t ld,
                      double q, int negate, double *thresh_dev, double *seas_dev,
                      int64_t ldo, void *stream);
int xmhw_clim_raw_f64(xmhw_plan *plan, const double *ts_dev, int64_t C, int64_t ld,
                      double q, int negate, double *thresh_dev, double *seas_dev,
                      int64_t ldo, void *stream);
/* The same on an int16-PACKED series read in place (CF packing: value = code * scale_factor + add_offset, `_FillValue`
 * -> NaN; what xr.open_dataset() decodes before threshold() sees it, docs/gettingstarted.rst:30-33): no decoded copy of
 * the series in HBM (2 bytes per sample instead of 4 or 8) and no decode pass.  codes_dev[T][ld] int16 (big_endian != 0:
 * byte-swapped, netCDF classic); decoded_itemsize = the dtype xarray (and xmhw_decode) would decode to:
 *   4  float32 (float32 packing attributes): the result is bit-identical to xmhw_decode(..., float32) +
 *      xmhw_clim_raw_f32 -- the kernel keys and sums float(code) * sf + of, two float32 roundings;
 *   8  float64 (float64 attributes): code -> value is monotone, so the kernel selects on the codes and decodes the
 *      two selected codes and the mean of the codes in float64: thresh bit-identical to xmhw_decode(..., float64) +
 *      xmhw_clim_raw_f64, seas within rounding (<= 1e-12: an exact integer sum instead of 440 rounded additions) --
 *      at the float32 kernel's speed instead of the 64-bit-key kernel's.
 * has_scale == 0: the samples are the codes themselves.  Served by the sorted-list kernel only: w = 5, records of 9..48
 * tracks, q >= 0.85; otherwise XMHW_ERR_UNSUPPORTED (decode, then xmhw_clim_raw_f32 / _f64).                        */
int xmhw_clim_raw_i16(xmhw_plan *plan, const int16_t *codes_dev, int64_t C, int64_t ld, int big_endian,
                      int has_scale, double scale_factor, double add_offset, int has_fill, int32_t fill_code,
                      int decoded_itemsize, double q, int negate, double *thresh_dev, double *seas_dev,
                      int64_t ldo, void *stream);

/* xmhw_clim_finish: the Feb-29 substitution (feb29(), identify.py:137-151,
 * applied at :237-240/:265-268 when feb29_fix != 0, i.e. tstep False) and
 * the circular running mean (runavg(), identify.py:154-181, when smooth != 0;
 * smooth_width must be odd) on both arrays, per cell over the groups PRESENT
 * (non-NaN) for that cell, as the reference's per-cell series are.
 * in/out may not alias.                                                      */
int xmhw_clim_finish(const xmhw_plan *plan, const double *thresh_in_dev,
                     const double *seas_in_dev, int64_t C, int64_t ldo, int feb29_fix,
                     int smooth, int smooth_width, double *thresh_out_dev,
                     double *seas_out_dev, void *stream);

/* One synchronous call = calc_clim() (xmhw.py:250-307) for all cells:
 * raw + finish, device buffers, builds a throw-away plan from doy_host.
 * D must equal the number of distinct labels in doy_host.                    */
int xmhw_clim_f32(const float *ts_dev, const int32_t *doy_host, int64_t T, int64_t C,
                  int32_t D, int32_t window_half_width, double q, int smooth,
                  int smooth_width, int feb29_fix, int negate, double *thresh_dev,
                  double *seas_dev, void *stream);
int xmhw_clim_f64(const double *ts_dev, const int32_t *doy_host, int64_t T, int64_t C,
                  int32_t D, int32_t window_half_width, double q, int smooth,
                  int smooth_width, int feb29_fix, int negate, double *thresh_dev,
                  double *seas_dev, void *stream);
/* Same with HOST buffers (copies in and out; PCIe-inclusive).                */
int xmhw_clim_host_f32(const float *ts_host, const int32_t *doy_host, int64_t T, int64_t C,
                       int32_t D, int32_t window_half_width, double q, int smooth,
                       int smooth_width, int feb29_fix, int negate, double *thresh_host,
                       double *seas_host);
int xmhw_clim_host_f64(const double *ts_host, const int32_t *doy_host, int64_t T, int64_t C,
                       int32_t D, int32_t window_half_width, double q, int smooth,
                       int smooth_width, int feb29_fix, int negate, double *thresh_host,
                       double *seas_host);

/* land_check()'s dropna (identify.py:522-525) on the stacked array:
 * keep[c] = 0 if cell c is all-NaN (anynans != 0: has any NaN), else 1.      */
int xmhw_land_mask_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, int anynans,
                       uint8_t *keep_dev, void *stream);
int xmhw_land_mask_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, int anynans,
                       uint8_t *keep_dev, void *stream);

/* the same on int16 codes (packed input read in place, xmhw_clim_raw_i16): a sample is missing when its code is
 * fill_code (has_fill == 0: no cell is dropped); big_endian: the codes are byte-swapped                         */
int xmhw_land_mask_i16(const int16_t *codes_dev, int64_t T, int64_t C, int64_t ld, int big_endian, int has_fill,
                       int32_t fill_code, int anynans, uint8_t *keep_dev, void *stream);

/* land_check()'s compaction on resident data: out[r][c] = in[r][index[c]] for the
 * n ocean cells listed in index_dev (ascending stacked-cell numbers, int64), and
 * the inverse for the results (what unstack('cell') does, xmhw.py:210-214):
 * out[r][index[c]] = in[r][c], every other element of out[rows][ld_out] = NaN.  */
int xmhw_gather_cells_f32(const float *in_dev, int64_t rows, int64_t ld_in,
                          const int64_t *index_dev, int64_t n, float *out_dev, int64_t ld_out,
                          void *stream);
int xmhw_gather_cells_f64(const double *in_dev, int64_t rows, int64_t ld_in,
                          const int64_t *index_dev, int64_t n, double *out_dev, int64_t ld_out,
                          void *stream);
int xmhw_gather_cells_i16(const int16_t *in_dev, int64_t rows, int64_t ld_in,
                          const int64_t *index_dev, int64_t n, int16_t *out_dev, int64_t ld_out,
                          void *stream);
int xmhw_scatter_cells_f64(const double *in_dev, int64_t rows, int64_t ld_in,
                           const int64_t *index_dev, int64_t n, double *out_dev, int64_t ld_out,
                           void *stream);

/* ---- detect() front end (next row of the path) ---------------------- *
 * For every cell: bthresh[t] = ts[t] > thresh[row_of_t[t]] (define_events(),
 * identify.py:366-372; NaN compares false; negate != 0 works on -ts, xmhw.py:413-414),
 * then mhw_filter() (identify.py:415-479) with join_gaps()/join_events() (identify.py:273-325,
 * :532-536).  row_of_t_host[T]: index of each step's doy label among the rows of thresh (HOST).
 * Outputs are int32 [T][ldo] with -1 where the reference has NaN: events = label (start
 * position) of the event covering a step; start = start label stored at the END step of the
 * first member of a joined event; end = end step stored at the end step of its last member.
 * bthresh_dev (uint8 [T][ldo]) and nevents_dev (int32 [C], number of joined events per
 * cell) may be NULL.                                                                    */
int xmhw_detect_events_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                           const double *thresh_dev, int64_t ldt, const int32_t *row_of_t_host,
                           int32_t min_duration, int32_t join_gaps, int32_t max_gap, int32_t negate,
                           int32_t *events_dev, int32_t *start_dev, int32_t *end_dev,
                           uint8_t *bthresh_dev, int64_t ldo, int32_t *nevents_dev, void *stream);
int xmhw_detect_events_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                           const double *thresh_dev, int64_t ldt, const int32_t *row_of_t_host,
                           int32_t min_duration, int32_t join_gaps, int32_t max_gap, int32_t negate,
                           int32_t *events_dev, int32_t *start_dev, int32_t *end_dev,
                           uint8_t *bthresh_dev, int64_t ldo, int32_t *nevents_dev, void *stream);

/* Number of (joined) events per cell: nevents_dev[C] int32, from the start array of
 * xmhw_detect_events_* (one start per event).                                            */
int xmhw_count_events(const int32_t *start_dev, int64_t T, int64_t C, int64_t ldo,
                      int32_t *nevents_dev, void *stream);

/* Per-event statistics: mhw_df() (xmhw/features.py:22-70) and
 * mhw_features() (features.py:72-315) for every event of every cell, from the labels of
 * xmhw_detect_events_*.  seas/thresh are the (D, C) climatologies (re-expanded by
 * row_of_t_host as in define_events(), identify.py:366-368); offsets_dev[C+1] int64 is the
 * exclusive prefix sum of the per-cell event counts; table_dev[offsets[C]][XMHW_EVENT_COLUMNS]
 * float64 receives one row per event, cells in order, events of a cell in time order.
 * Columns (time stamps as positions along the time axis):
 *  0 event  1 index_start  2 index_end  3 time_start  4 time_end  5 time_peak
 *  6 intensity_max  7 intensity_mean  8 intensity_cumulative  9 severity_max
 * 10 severity_mean 11 severity_cumulative 12 severity_var 13 intensity_mean_relThresh
 * 14 intensity_cumulative_relThresh 15 intensity_mean_abs 16 intensity_cumulative_abs
 * 17 duration_moderate 18 duration_strong 19 duration_severe 20 duration_extreme
 * 21 index_peak 22 intensity_var 23 intensity_max_relThresh 24 intensity_max_abs
 * 25 intensity_var_relThresh 26 intensity_var_abs 27 category 28 duration
 * 29 rate_onset 30 rate_decline                                                          */
#define XMHW_EVENT_COLUMNS 31
int xmhw_event_stats_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                         const double *seas_dev, const double *thresh_dev, int64_t ldc,
                         const int32_t *row_of_t_host, int32_t negate, const int32_t *events_dev,
                         int64_t ldo, const int64_t *offsets_dev, double *table_dev, void *stream);
int xmhw_event_stats_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                         const double *seas_dev, const double *thresh_dev, int64_t ldc,
                         const int32_t *row_of_t_host, int32_t negate, const int32_t *events_dev,
                         int64_t ldo, const int64_t *offsets_dev, double *table_dev, void *stream);

/* define_events() (xmhw/identify.py:326-412) when only the event TABLE is wanted — no per-step
 * outputs, the least HBM traffic the result allows.  Three stages:
 *  1. xmhw_exceed_bits_*: ts > thresh[row(t)] (identify.py:366-372) as one bit per sample;
 *     bits_dev [ceil(T/64)][ldb] uint64, bit (t & 63) of word t/64 of column c.  thresh_dev
 *     is (D, ldt); the f32 variant compares against the float32 floor of each threshold
 *     (identical results, half the bytes re-read per step).
 *  2. xmhw_events_from_bits: mhw_filter() + join_gaps() (identify.py:415-479, 273-325) on the
 *     bits.  offsets_dev == NULL: count only, nevents_dev[C] = events per cell.  Otherwise
 *     (offsets_dev[C+1] = exclusive prefix sum of those counts) column 0 (label), 1 (cell
 *     index, scratch), 3 and 4 (first / last labelled step) of every event's row of
 *     table_dev[offsets[C]][XMHW_EVENT_COLUMNS] are written; nevents_dev may be NULL.
 *     Asynchronous on `stream`.
 *  3. xmhw_event_stats_sparse_*: mhw_df() + mhw_features() (xmhw/features.py:22-315) for the
 *     n_events rows prepared by stage 2, one thread per event; fills all 31 columns.
 * Same results as xmhw_detect_events_* + xmhw_event_stats_*.                              */
/* Kernel choice of xmhw_exceed_bits_* (process-wide; tests and measurements): 0 = automatic
 * (tiled kernel - thresholds read once per cell - for calendar-like labels on >= 131072 cells,
 * otherwise the per-step kernel), 1 = per-step kernel, 2 = tiled kernel.                     */
int xmhw_set_exceed_kernel(int32_t mode);
int xmhw_exceed_bits_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                         const double *thresh_dev, int64_t ldt, int64_t D,
                         const int32_t *row_of_t_host, int32_t negate, uint64_t *bits_dev,
                         int64_t ldb, void *stream);
int xmhw_exceed_bits_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                         const double *thresh_dev, int64_t ldt, int64_t D,
                         const int32_t *row_of_t_host, int32_t negate, uint64_t *bits_dev,
                         int64_t ldb, void *stream);
int xmhw_events_from_bits(const uint64_t *bits_dev, int64_t T, int64_t C, int64_t ldb,
                          int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                          const int64_t *offsets_dev, int32_t *nevents_dev, double *table_dev,
                          void *stream);
int xmhw_event_stats_sparse_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                                const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                const int32_t *row_of_t_host, int32_t negate, int64_t n_events,
                                double *table_dev, void *stream);
int xmhw_event_stats_sparse_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                                const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                const int32_t *row_of_t_host, int32_t negate, int64_t n_events,
                                double *table_dev, void *stream);

/* The `intermediate` Dataset of detect() (xmhw/xmhw.py:354-356; define_events(),
 * identify.py:405-409): the per-step columns mhw_df() adds (xmhw/features.py:36-69).
 * out_dev [8][T][ldv] float64 = seas, thresh (NaN outside events), relSeas, relThresh,
 * relThreshNorm, severity, cats, mabs; dur_dev [4][T][ldv] uint8 = duration_moderate,
 * duration_strong, duration_severe, duration_extreme.                                    */
#define XMHW_INTERMEDIATE_F64_PLANES 8
#define XMHW_INTERMEDIATE_U8_PLANES 4
int xmhw_event_intermediate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                                const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                const int32_t *row_of_t_host, int32_t negate,
                                const int32_t *events_dev, int64_t ldo, double *out_dev,
                                int64_t ldv, uint8_t *dur_dev, void *stream);
int xmhw_event_intermediate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                                const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                const int32_t *row_of_t_host, int32_t negate,
                                const int32_t *events_dev, int64_t ldo, double *out_dev,
                                int64_t ldv, uint8_t *dur_dev, void *stream);

/* Synthetic SST generated in HBM (bench + large parity runs):
 * x[t,c] = 15 + A_c sin(2 pi (t - phi_c)/365.25) + 5e-4 t beta_c + N(0,1),
 * counter-based on (seed, cell0 + c, t); a sample is NaN with probability
 * nan_frac.                                                                  */
int xmhw_synth_sst_f32(float *ts_dev, int64_t T, int64_t C, int64_t ld, int64_t cell0,
                       uint64_t seed, double nan_frac, void *stream);
int xmhw_synth_sst_f64(double *ts_dev, int64_t T, int64_t C, int64_t ld, int64_t cell0,
                       uint64_t seed, double nan_frac, void *stream);
/* the same with what real archives add (bench legs): values rounded to multiples of `quant` (OISST: 0.01; 0 = off), a
 * share `ice_frac` of the cells held at -1.8 for 120 days of every year, AR(1) anomalies with day-to-day correlation
 * `rho` (unit variance; 0 = the white noise of xmhw_synth_sst_f32, to which this is then bit-identical).  ice_patch:
 * the ice cells come in patches of that many consecutive cells with one season start per patch and +-15 days per cell
 * (an ice pack: neighbours freeze together); <= 1 = every cell decides and freezes on its own (scattered: the worst
 * case for a kernel that runs 32 neighbouring cells in lockstep)                                                     */
int xmhw_synth_sst_ex_f32(float *ts_dev, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed,
                          double nan_frac, double quant, double ice_frac, double rho, int64_t ice_patch,
                          void *stream);

/* The detect-side entries above take host row tables (row_of_t).  Their device copies (and the tiled
 * exceedance kernel's chunk tables, and per-stream scratch such as the float32 threshold copy) are
 * CACHED between calls, keyed by content: after the first call with a given table the entries are
 * asynchronous on `stream` -- no allocation, no synchronisation.  xmhw_release_cached_tables() frees
 * the caches (synchronises the device).
 * xmhw_offsets_from_counts: exclusive prefix sum of the per-cell event counts (the count pass of
 * xmhw_events_from_bits) into the int64 offsets (n + 1 entries, the last one = number of events)
 * the fill pass takes -- on the device, asynchronous.                                           */
int xmhw_release_cached_tables(void);
int xmhw_offsets_from_counts(const int32_t *counts_dev, int64_t n, int64_t *offsets_dev, void *stream);

/* ---- block_average() (xmhw/stats.py:27-428) ------------------------------ *
 * The reference runs groupby(pd.cut(years, bins, right=False)).agg(...) per cell (call_groupby
 * :285-319).  Device buffers throughout; bin_of_t[T] (int32, device) = year-bin index of every time
 * step, -1 outside the bins.  Results: out[stat][bin][cell] float64, leading dimension ldo >= C.
 * xmhw_block_events: the 15 statistics of agg_mhw (:344-362: ecount, duration, intensity_max,
 * intensity_max_max, intensity_mean, intensity_cumulative, total_icum, intensity_mean_relThresh,
 * intensity_cumulative_relThresh, severity_mean, severity_cumulative, intensity_mean_abs,
 * intensity_cumulative_abs, rate_onset, rate_decline) from the compact event table of detect()
 * (n_events x 31, events of cell c at rows offsets[c]..offsets[c+1]); an event belongs to the bin
 * of the time step in column mtime_column (3 = time_start, 5 = time_peak).
 * xmhw_block_time_*: ts_mean, ts_max, ts_min per block (agg_ts :421-425) and, when `cats` (T, ldcat)
 * is given, the moderate / strong / severe / extreme day counts (agg_cats :391-400): 7 planes.  */
int xmhw_block_events(const double *table_dev, const int64_t *offsets_dev, int64_t C,
                      const int32_t *bin_of_t_dev, int64_t T, int32_t nbins, int32_t mtime_column,
                      double *out_dev, int64_t ldo, void *stream);
int xmhw_block_time_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *cats_dev,
                        int64_t ldcat, const int32_t *bin_of_t_dev, int32_t nbins, double *out_dev,
                        int64_t ldo, void *stream);
int xmhw_block_time_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *cats_dev,
                        int64_t ldcat, const int32_t *bin_of_t_dev, int32_t nbins, double *out_dev,
                        int64_t ldo, void *stream);

/* ---- mhw_rank() (xmhw/stats.py:446-510) ------------------------------------------------------ *
 * Per-cell ranks and return periods of event properties, on the compact event table of detect()
 * (table_dev row-major with leading dimension ld_table; the events of cell c are rows
 * offsets_dev[c]..offsets_dev[c+1]).  For column k of the list (columns[k] < ld_table, host array,
 * 1 <= ncols <= 31) and event i of a cell, over the values v of that column in that cell:
 *     rank_i = 1 + #{j : v_j > v_i} + #{j > i : v_j == v_i}
 * i.e. the largest value has rank 1 and of equal values the later event ranks first
 * (= N - argsort(argsort(v, kind="stable")) over the N non-NaN values); values compare as float64,
 * so -0.0 == 0.0.  A NaN value gets a NaN rank and does not count for the other events.
 * Return period rp_i = (n_years + 1) / rank_i (one float64 division; NaN where the rank is NaN),
 * n_years finite and > 0.  Results go to rank_dev / rp_dev [row][ld_out] at column k (ld_out >= ncols);
 * no other element is written.  Asynchronous on `stream`; nothing is launched for C == 0.        */
int xmhw_event_rank(const double *table_dev, int64_t ld_table, const int64_t *offsets_dev, int64_t C,
                    const int32_t *columns, int32_t ncols, double n_years, double *rank_dev, double *rp_dev,
                    int64_t ld_out, void *stream);

/* ---- mean_trend() (Oliver's marineHeatWaves.meanTrend(); not in xmhw) -------------------------- *
 * Per (cell, statistic) trends of the planes of block_average(): y_dev[stat][block][ld] float64, cells
 * contiguous (ld >= C), nstat x nb x C items' worth.  x_dev[nb]: the abscissa, years centred on the
 * whole period, STRICTLY INCREASING (not checked: it lives on the device).  A NaN block is left out of
 * its series (m = the valid blocks of an item); an item with a valid +-Inf, or with m == 0, is NaN in
 * every output.  Outputs are planes out_dev[what][stat][ldo] (ldo >= C); elements at columns >= C are
 * not written.  Asynchronous on `stream`; nothing is launched for nstat == 0 or C == 0; nb == 0 gives
 * NaN everywhere.  No FMA contraction, sums in block order: results are the same from run to run.
 *
 * xmhw_block_trend_ols: what = 0 mean, 1 trend, 2 dtrend.  Least squares of y on [1, x] over the valid
 * blocks: xb = sum(x)/m, yb = sum(y)/m, Sxx = sum((x-xb)^2), Sxy = sum((x-xb)(y-yb)), trend = Sxy/Sxx,
 * mean = yb - trend*xb (the fit at x = 0), r = y - (mean + trend*x), s = sqrt(sum(r^2)/(m-2)),
 * dtrend = tcrit[m-2]*s/sqrt(Sxx).  tcrit_dev[k], k = 1..nb-2: the two-sided Student-t critical value
 * for k degrees of freedom (nb - 1 entries, entry 0 unused; may be NULL for nb < 3).  m == 1: mean = y,
 * trend and dtrend NaN; m == 2: dtrend NaN.
 *
 * xmhw_block_trend_theil_sen: what = 0 trend, 1 mean, 2 mk_s, 3 mk_var.  Over the pairs i < j of valid
 * blocks, N = m(m-1)/2: trend = the median (s[(N-1)/2] + s[N/2])/2 of the slopes (y_j-y_i)/(x_j-x_i)
 * sorted in IEEE total order; mean = median(y) - trend*median(x) over the valid blocks; mk_s =
 * sum sign(y_j - y_i) (Mann-Kendall S); mk_var = (m(m-1)(2m+5) - sum_b (c_b-1)(2c_b+5))/18 with
 * c_b = #{j: y_j == y_b}, the tie-corrected variance (integer numerator, one division).  m < 2: trend
 * NaN (mean = y for m == 1); m < 3: mk_s and mk_var NaN.  nb above 128 blocks: XMHW_ERR_UNSUPPORTED.  */
int xmhw_block_trend_ols(const double *y_dev, int32_t nstat, int32_t nb, int64_t C, int64_t ld,
                         const double *x_dev, const double *tcrit_dev, double *out_dev, int64_t ldo,
                         void *stream);
int xmhw_block_trend_theil_sen(const double *y_dev, int32_t nstat, int32_t nb, int64_t C, int64_t ld,
                               const double *x_dev, double *out_dev, int64_t ldo, void *stream);

/* ---- detrend(): per-cell trend fit and removal on the resident series (not in xmhw / marineHeatWaves) -- *
 * ts_dev (T, C) float32 / float64, time-major, cells contiguous (ld >= C).  basis_dev[T][P] float64: the
 * design matrix, one row per step, shared by all cells (xmhw_amd/detrend.py builds it: powers of the time
 * in decades since a reference, the constant, annual harmonics).  weight_dev[T] uint8 in {0, 1}: the steps
 * of the fit period (NULL: all of them).  A sample CONTRIBUTES when its step has weight 1 and it is not NaN.
 *
 * xmhw_series_fit_*: coef_dev[k][ldc] (ldc >= C), k < P: the least-squares solution over the contributing
 * samples of every cell -- normal equations G = sum b b', r = sum b y accumulated in float64 in time order
 * (r in batches of eight steps that join the running sum by a compensated add, the shared Gram matrix by a
 * compensated sum), Cholesky with the columns in the order of the basis, two triangular solves; no FMA.  (The
 * Gram matrix of the steps with weight 1 is summed once per call; a cell takes it less the outer products of
 * its own missing steps, or -- when more of its samples are missing than contribute -- sums its own.)  A cell
 * FAILS, and all its coefficients are NaN, when it has fewer than max(min_valid, P) contributing samples,
 * when a contributing sample is +-Inf, or when a pivot d_j = G_jj - sum_k L_jk^2 is not > 1e-6 * G_jj (NaN
 * and negative pivots included).  nvalid_dev[C] (may be NULL): the contributing samples of every cell.
 * A cell's result depends on its own samples only -- not on C, ld or the launch -- and is the same from run
 * to run.  1 <= P <= XMHW_FIT_MAX_TERMS, above: XMHW_ERR_UNSUPPORTED and nothing is written.
 *
 * xmhw_series_remove_*: in place, for every step, y' = y - sum_{k<R} coef[k] basis[t][k]: the sum in float64
 * in column order, one subtraction in float64, one rounding to the sample type.  1 <= R <= P: the leading
 * columns are removed, the others were fitted and stay.  NaN stays NaN; a failed cell becomes NaN everywhere.
 *
 * Both are asynchronous on `stream`; nothing is launched for C == 0 or T == 0; elements at columns >= C of
 * ts_dev, coef_dev and nvalid_dev are never touched.  Scratch: 512 + C bytes of the stream's scratch buffer.
 * xmhw_series_remove_* takes at most 65535 * 64 steps (above: XMHW_ERR_UNSUPPORTED).                          */
#define XMHW_FIT_MAX_TERMS 10
int xmhw_series_fit_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *basis_dev,
                        int32_t P, const uint8_t *weight_dev, int32_t min_valid, double *coef_dev,
                        int64_t ldc, int32_t *nvalid_dev, void *stream);
int xmhw_series_fit_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *basis_dev,
                        int32_t P, const uint8_t *weight_dev, int32_t min_valid, double *coef_dev,
                        int64_t ldc, int32_t *nvalid_dev, void *stream);
int xmhw_series_remove_f32(float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *basis_dev,
                           int32_t P, int32_t R, const double *coef_dev, int64_t ldc, void *stream);
int xmhw_series_remove_f64(double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *basis_dev,
                           int32_t P, int32_t R, const double *coef_dev, int64_t ldc, void *stream);

/* ---- mhw_coverage(): daily area in each MHW category, by region (Hobday et al. 2018, fig. 3) ------ *
 * The one reduction ACROSS cells.  For every step t of the dense series ts_dev (T, C) and every region
 * r < R, ADDS to cells_dev[t][r][k] the number of cells c with region_dev[c] == r that are in state k on
 * step t, and to area_q_dev[t][r][k] the sum of their weights wq_dev[c]; both [T][R][5] int64, contiguous,
 * zeroed by the caller before the first slab of cells: calls for consecutive slabs accumulate, on the same
 * stream, without a read-back in between.  States k: 0 moderate, 1 strong, 2 severe, 3 extreme, 4 event.
 * A step is "in an event" iff detect() labels it: mhw_filter() + join_gaps() (xmhw/identify.py:415-479,
 * 273-325) on bits_dev, the exceedance words written by xmhw_exceed_bits_* for the same slab (ldb >= C);
 * the walk is the one of xmhw_events_from_bits.  Its category is the per-step one of mhw_df()
 * (xmhw/features.py:52-66): cats = floor(1 + (ts - thresh)/(thresh - seas)) in float64 with seas / thresh
 * re-expanded by row_of_t_host; k = 0..3 for cats == 1, == 2, == 3, >= 4.  A step inside a joined gap
 * (below the threshold, or NaN) is in an event and in none of the four, so column 4 >= the sum of 0..3.
 * negate != 0: the series is negated first (cold spells).
 * region_dev[C] int32 in [-1, R): -1 = the cell counts nowhere.  wq_dev[C] int64, 0 <= wq <= 2^31 (not
 * checked: it lives on the device): with C < 2^32 no sum can overflow.  All sums are integer sums: the
 * result is exact and does not depend on the order of the adds, the slabs or the launch geometry.
 * R >= 1; R above XMHW_COVERAGE_MAX_REGIONS: XMHW_ERR_UNSUPPORTED.  Asynchronous on `stream`; nothing is
 * launched for C == 0.  Scratch: one in-event bit per sample, in the stream's scratch buffer.           */
#define XMHW_COVERAGE_MAX_REGIONS 1024
#define XMHW_COVERAGE_STATES 5
int xmhw_coverage_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld,
                                 const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                 const int32_t *row_of_t_host, int32_t negate, const uint64_t *bits_dev,
                                 int64_t ldb, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                                 const int64_t *wq_dev, const int32_t *region_dev, int32_t R,
                                 int64_t *cells_dev, int64_t *area_q_dev, void *stream);
int xmhw_coverage_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld,
                                 const double *seas_dev, const double *thresh_dev, int64_t ldc,
                                 const int32_t *row_of_t_host, int32_t negate, const uint64_t *bits_dev,
                                 int64_t ldb, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                                 const int64_t *wq_dev, const int32_t *region_dev, int32_t R,
                                 int64_t *cells_dev, int64_t *area_q_dev, void *stream);

/* ---- region_series(): the area-weighted mean series of every region (box, basin, EEZ, index area) ---- *
 * The reduction ACROSS cells that sums values.  For every step t of the dense series ts_dev (T, C), leading
 * dimension ld, and every region r < R, ADDS into the contiguous accumulator acc_dev[T][R][3] (int64), over
 * the cells c with region_dev[c] == r whose sample at t is not NaN:
 *   acc[t][r][0] (n_valid) += 1
 *   acc[t][r][1] (wsum_i)  += wi_dev[c]
 *   acc[t][r][2] (xsum_q)  += wi_dev[c] * xq,  xq = rint(((double)ts[t][c] - x0) * 2^XMHW_REGION_SERIES_BITS)
 * xq is computed in float64 exactly as written (the product by 2^16 is exact, rint rounds half to even), so
 * numpy.rint((ts.astype(float64) - x0) * 65536.0) is the same integer for every sample.  xsum_q is signed, held
 * in two's complement in the 64-bit adds.  A valid sample with |ts - x0| >= 2^7, or infinite, is left out of
 * all three sums and counted in *n_range_dev (int64, ADDED to as well; 0 for data in range: pass x0 = 273.15
 * for a series in kelvin).  region_dev[C] int32 in [-1, R): -1 = the cell counts nowhere (its samples are not
 * read).  wi_dev[C] int64, 0 <= wi <= 2^ib with ib <= 61 - 16 - 7 - bit_length(cells of the whole grid) (not
 * checked: it lives on the device): |xsum_q| <= C * 2^(ib + 23) < 2^61 whatever the data.
 * The caller zeroes acc_dev and *n_range_dev before the first slab of cells: calls for consecutive slabs
 * accumulate, on the same stream, without a read-back in between.  All sums are integer sums: the result is
 * exact and does not depend on the order of the adds, the slabs or the launch geometry.
 * R >= 1; R above XMHW_REGION_MAX_REGIONS: XMHW_ERR_UNSUPPORTED, before anything is touched.  Asynchronous on
 * `stream`; nothing is launched for C == 0 or T == 0.  xmhw_set_region_wave_sum (process-wide; tests and
 * measurements): how a wave sums its 64-bit terms, 1 = the sums of 8 steps together (the default), 0 = one
 * wave sum per step.  Same results.                                                                   */
#define XMHW_REGION_MAX_REGIONS 1024
#define XMHW_REGION_SERIES_BITS 16
int xmhw_set_region_wave_sum(int32_t variant);
int xmhw_region_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, double x0,
                               const int64_t *wi_dev, const int32_t *region_dev, int32_t R,
                               int64_t *acc_dev /* [T][R][3] */, int64_t *n_range_dev, void *stream);
int xmhw_region_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, double x0,
                               const int64_t *wi_dev, const int32_t *region_dev, int32_t R,
                               int64_t *acc_dev /* [T][R][3] */, int64_t *n_range_dev, void *stream);

/* ---- mhw_objects(): the events of detect() grouped into objects connected in space and time -------- *
 * A table row r is a run of days start_dev[r]..end_dev[r] (inclusive positions along the time axis, int32)
 * in one ocean cell; the rows of cell c are offsets_dev[c]..offsets_dev[c+1] (offsets_dev[C] == n), in time
 * order and at least one day apart (not checked: they live on the device).  nbr_dev[C][K] int32 lists the
 * spatial neighbours of every cell as cell numbers, -1 = none (land, outside the grid); the relation must be
 * symmetric and a cell is not its own neighbour.  Rows a, b of DIFFERENT cells are linked iff one cell is a
 * neighbour of the other and start_a <= end_b + gap and start_b <= end_a + gap (gap 0: the runs share a day,
 * 6-connectivity of the voxels; gap 1: they may also be a day apart, 26-connectivity with K = 8).
 *
 * xmhw_event_objects writes cell_of_row_dev[n] (the cell of every row) and root_dev[n]: the SMALLEST row of
 * the row's connected component, whatever the schedule (a lock-free union-find; no wave waits for another).
 * n or C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  Nothing is launched for n == 0.
 *
 * xmhw_object_reduce reduces the rows into per-object slots: slot_dev[r] in [0, n_slots) is equal for the rows
 * of one object (root_dev with n_slots = n serves; a row whose slot is outside the range is left out).  It
 * initialises and fills, for every slot: n_events (rows), n_cells (distinct cells), time_start = min start,
 * time_end = max end, cell_days = sum (end - start + 1), area_days_q = sum wq_dev[cell] * (end - start + 1)
 * (wq_dev[C] int64 >= 0; the caller sizes it so that no sum passes 2^63), intensity_max = the largest
 * imax_dev[r] compared as float64 with -0.0 counted as 0.0, NaN rows ignored (NaN if there is none), and
 * peak_row = the smallest row that attains it (-1 if none).  A slot without rows keeps 0, 0, 2^31-1, -1, 0,
 * 0, NaN, -1.  Only integer sums, minima and maxima: the result is exact and the same from run to run.
 * Both are asynchronous on `stream`.                                                                        */
int xmhw_event_objects(const int32_t *start_dev, const int32_t *end_dev, int64_t n, const int64_t *offsets_dev,
                       int64_t C, const int32_t *nbr_dev, int32_t K, int32_t gap, int32_t *cell_of_row_dev,
                       int32_t *root_dev, void *stream);
int xmhw_object_reduce(const int32_t *start_dev, const int32_t *end_dev, const double *imax_dev, int64_t n,
                       const int32_t *cell_of_row_dev, const int64_t *offsets_dev, const int64_t *wq_dev,
                       const int32_t *slot_dev, int64_t n_slots, int32_t *n_events_dev, int32_t *n_cells_dev,
                       int32_t *time_start_dev, int32_t *time_end_dev, int64_t *cell_days_dev,
                       int64_t *area_days_q_dev, double *intensity_max_dev, int32_t *peak_row_dev, void *stream);

/* ---- mhw_tracks(): the daily series of the objects (cells, area, first moments), ragged ------------- *
 * The rows are those of xmhw_object_reduce (start_dev, end_dev, cell_of_row_dev as xmhw_event_objects wrote it).
 * slot_dev[r] is the position of row r's object in the caller's SELECTION, in [0, n_slots); a row with any other
 * slot does nothing.  Selected object i lives from time_start_dev[i] to its last day and owns the entries
 * offsets_dev[i] .. offsets_dev[i + 1] - 1 of every series, one per day (offsets_dev[n_slots + 1] int64,
 * offsets_dev[0] == 0, offsets_dev[n_slots] == L = the sum of the durations).  vec_dev[4][ldv] int64 holds four
 * addends per cell (ldv >= C): mhw_tracks() passes the area weight wq and the moment terms wm*ux, wm*uy, wm*uz.
 *
 * Initialises and fills n_cells_dev[L + 1] int32 and sums_dev[4][ld] int64 (ld >= L + 1): entry
 * offsets[i] + (t - time_start[i]) of n_cells is the number of rows of object i that cover day t (one per cell:
 * the rows of a cell are disjoint), and of sums[k] the sum of vec[k][cell] over them.  Entry L of all five is a
 * sentinel that ends as 0.  Method: every row adds its vector at its first day and subtracts it behind its last
 * (integer atomics; a row that ends on its object's last day puts the negative term on the next object's first
 * entry, or on the sentinel), then ONE inclusive scan of the whole array, in place, as reduce-then-scan over tiles
 * of XMHW_TRACKS_TILE entries in separate launches.  No kernel waits for another workgroup; sums wrap modulo 2^64
 * on the way and are exact whenever the true values fit int64 (int32 for n_cells).  The result is the same from
 * run to run.  *n_bad_dev (one int32) counts the rows left out because their days fall outside their object's
 * entries or their cell outside [0, C): 0 for consistent inputs; nothing outside entries 0..L is written.
 * n, n_slots or L + 1 of 2^31 and more: XMHW_ERR_UNSUPPORTED (select fewer objects).  Scratch for the tile sums
 * comes from the stream's scratch buffer.  Asynchronous on `stream`.                                         */
#define XMHW_TRACKS_TILE 1024
int xmhw_object_tracks(const int32_t *start_dev, const int32_t *end_dev, int64_t n, const int32_t *slot_dev,
                       const int32_t *cell_of_row_dev, int64_t C, const int64_t *vec_dev, int64_t ldv,
                       const int32_t *time_start_dev, const int64_t *offsets_dev, int64_t n_slots, int64_t L,
                       int32_t *n_cells_dev, int64_t *sums_dev, int64_t ld, int32_t *n_bad_dev, void *stream);

/* ---- mhw_track_parts(): the connected parts of every object on each of its days, ragged -------------- *
 * The rows and the ragged layout are those of xmhw_object_tracks: start_dev / end_dev / slot_dev / cell_of_row_dev
 * [n] int32, slot in [0, n_slots) = the position of the row's object in the selection (any other slot: the row does
 * nothing), selected object i owns the entries offsets_dev[i] .. offsets_dev[i + 1] - 1, one per day from
 * time_start_dev[i]; offsets_dev[n_slots] == L.  The rows of cell c are row_offsets_dev[c] .. row_offsets_dev[c + 1]
 * (int64[C + 1]), in time order, as for xmhw_event_objects; nbr_dev[C][K] int32 lists every cell's spatial neighbours
 * (-1: none; symmetric, a cell is not its own neighbour; K = 4 or 8 in mhw_track_parts()).  wq_dev[C] int64 >= 0.
 *
 * The footprint of object i on day t is the set of cells holding a row of slot i with start <= t <= end; two
 * footprint cells are adjacent iff one is among the other's neighbours; a part is a connected component.  Rows of
 * different slots are never joined, whatever nbr says.  Entry offsets[i] + (t - time_start[i]) receives n_parts
 * (int32, the number of parts), cells_largest (int32, the most cells in one part) and area_largest_q (int64, the
 * largest sum of wq over one part).  The two maxima are independent: they may come from different parts.
 *
 * Voxels.  vox_off_dev[n + 1] int64 is the exclusive prefix sum of end - start + 1 over the rows with a slot in
 * [0, n_slots), 0 for the others; V = vox_off_dev[n], given by the caller; day t of row r is voxel vox_off[r] + t -
 * start[r].  SCRATCH: XMHW_PARTS_VOXEL_BYTES (16) per voxel -- parent int32, cells int32, area int64 -- taken from
 * the stream's scratch buffer, as in xmhw_coverage_accumulate_*; the caller passes none.
 *
 * Method, five launches on `stream`: parent[v] = v and the outputs zeroed; lane = row: for every neighbour cell with a
 * smaller number, the rows of that cell that overlap the lane's in time and have its slot are found by a binary search
 * and a walk, and the two voxels of every common day are united by the lock-free union-find of xmhw_event_objects
 * (the smaller root wins by compare-and-swap; no wave waits for another); the roots are flattened; every voxel adds 1
 * and wq[cell] to its root (integer atomics); every root adds 1 to n_parts and raises the two maxima of its entry
 * (integer atomic maxima, the area as unsigned 64-bit).  Exact, and the same from run to run.
 * A selected row whose days leave its object's entries, whose cell is outside [0, C) or whose voxel numbers are not
 * vox_off[r] .. vox_off[r + 1] - 1 within [0, V) is left out and counted in *n_bad_dev (int32; 0 for consistent
 * inputs): nothing outside entries 0..L-1 and voxels 0..V-1 is ever written.  n, C, n_slots, L or V of 2^31 and more:
 * XMHW_ERR_UNSUPPORTED (select fewer objects).  Asynchronous on `stream`.                                   */
#define XMHW_PARTS_VOXEL_BYTES 16
int xmhw_object_parts(const int32_t *start_dev, const int32_t *end_dev, const int32_t *slot_dev,
                      const int32_t *cell_of_row_dev, int64_t n, const int64_t *row_offsets_dev, int64_t C,
                      const int32_t *nbr_dev, int32_t K, const int64_t *wq_dev, const int64_t *vox_off_dev, int64_t V,
                      const int32_t *time_start_dev, const int64_t *offsets_dev, int64_t n_slots, int64_t L,
                      int32_t *n_parts_dev, int32_t *cells_largest_dev, int64_t *area_largest_q_dev,
                      int32_t *n_bad_dev, void *stream);

/* ---- mhw_track_genealogy(): the links between the parts of consecutive days of every object ----------- *
 * The rows, the ragged layout, the neighbour table, the voxels and the parts are those of xmhw_object_parts (no
 * weights).  Part A of day t - 1 and part B of day t of one selected object are linked iff some cell lies in A on
 * t - 1 and in B on t (overlap; a neighbouring cell does not link).  The distinct links are the edges of the
 * genealogy; the in-degree of a part counts its links to the day before, its out-degree those to the day after.
 * counts_dev[XMHW_GENEALOGY_FIELDS][L] int32, one array of L entries per field in the order of the XMHW_GENEALOGY_*
 * indices: entry offsets[i] + (t - time_start[i]) receives, over the parts of object i on day t, their number, the sum
 * of their in-degrees, the parts of in-degree 0, of in-degree >= 2, of out-degree 0 and of out-degree >= 2.
 * edges_dev[edge_capacity] uint64 receives the *n_edges_dev (int64) edges as (root of A << 32) | root of B in ARBITRARY
 * order; the root of a part is its smallest voxel number, a voxel of its smallest cell: the caller finds row, day and
 * cell of a root by a search of vox_off.  edge_capacity must be at least the number of (row, day) pairs of the selected
 * rows that have a next day in the same row, plus the pairs of consecutive rows of one cell and one slot with
 * start == end + 1: then the hash set below is never more than half full.
 *
 * SCRATCH, from the stream's scratch buffer: XMHW_GENEALOGY_VOXEL_BYTES (12) per voxel -- parent, in-degree and
 * out-degree, int32 -- plus XMHW_GENEALOGY_SLOT_BYTES (8) per slot of a hash set whose capacity is the smallest power
 * of two >= 2 * max(edge_capacity, 1).
 *
 * Method, seven launches on `stream`: everything initialised (an empty slot is all ones; roots are below 2^31, so no
 * key equals it); the link and flatten passes of xmhw_object_parts; lane = row: for every day of the row but its last
 * the key (root today, root tomorrow), and the key across two touching rows of one cell and slot, inserted by linear
 * probing from a mixed hash with one 64-bit compare-and-swap per probe -- an empty slot taken makes the lane the one
 * winner of that distinct pair, which adds 1 to the two degrees; the same key found is a duplicate; another key sends
 * the lane to the next slot; the loop ends after `capacity` probes at the latest and then sets *overflow_dev (int32;
 * 0 whenever edge_capacity is as stated above); no lane waits for another; lane = slot: the slots in use are copied to
 * edges_dev, a wave taking its places with one atomic, nothing at or beyond edge_capacity written; lane = row: every
 * voxel that is its own root adds to the six counts of its entry (integer atomics).  Exact, and the same from run to
 * run once the edges are sorted.  Rows that do not fit are left out and counted in *n_bad_dev as in
 * xmhw_object_parts.  n, C, n_slots, L, V or edge_capacity of 2^31 and more: XMHW_ERR_UNSUPPORTED.  Asynchronous on
 * `stream`.                                                                                                */
#define XMHW_GENEALOGY_VOXEL_BYTES 12
#define XMHW_GENEALOGY_SLOT_BYTES 8
#define XMHW_GENEALOGY_FIELDS 6
#define XMHW_GENEALOGY_PARTS 0
#define XMHW_GENEALOGY_LINKS 1
#define XMHW_GENEALOGY_BORN 2
#define XMHW_GENEALOGY_MERGED 3
#define XMHW_GENEALOGY_ENDED 4
#define XMHW_GENEALOGY_SPLIT 5
int xmhw_object_genealogy(const int32_t *start_dev, const int32_t *end_dev, const int32_t *slot_dev,
                          const int32_t *cell_of_row_dev, int64_t n, const int64_t *row_offsets_dev, int64_t C,
                          const int32_t *nbr_dev, int32_t K, const int64_t *vox_off_dev, int64_t V,
                          const int32_t *time_start_dev, const int64_t *offsets_dev, int64_t n_slots, int64_t L,
                          int32_t *counts_dev, uint64_t *edges_dev, int64_t edge_capacity, int64_t *n_edges_dev,
                          int32_t *n_bad_dev, int32_t *overflow_dev, void *stream);

/* ---- mhw_track_shape(): the perimeter and the coast contact of every object on each of its days ------- *
 * The rows, the ragged layout and row_offsets_dev are those of xmhw_object_parts (no weights, no voxels, no
 * scratch).  Every cell has K = 4 faces, in the order dim 0 minus, dim 0 plus, dim 1 minus, dim 1 plus.
 * faces_dev[C][4] int32 names what lies across each: the compact cell there (>= 0; it may be the same cell for two
 * faces, on a wrapping dim of length 2), XMHW_SHAPE_FACE_COAST (a grid point that is no cell), XMHW_SHAPE_FACE_BORDER
 * (no grid point) or XMHW_SHAPE_FACE_FOLDED (a wrapping dim of length 1: no face, nothing is counted).
 * lq_dev[C][4] int64 >= 0 holds the lengths of the faces; the caller sizes them so that 4 * C * max(lq) < 2^63.
 *
 * The footprint of object i on day t is the set of cells holding a row of slot i with start <= t <= end.  A face of
 * a footprint cell to a cell of the same footprint is shared and counts nothing; a face to any other cell is OPEN; a
 * coast face is COAST, a border face BORDER.  Entry offsets[i] + (t - time_start[i]) receives, per class in the order
 * of the XMHW_SHAPE_* indices, edges_dev[XMHW_SHAPE_CLASSES][L] int32 (the number of such faces) and
 * perimeter_q_dev[XMHW_SHAPE_CLASSES][L] int64 (the sum of their lq), one array of L entries per class, and
 * cells_edge_dev[L] int32 (the footprint cells with at least one open, coast or border face).
 *
 * Method, on `stream`: the seven arrays and *n_bad_dev zeroed by memsets; one launch, lane = row: coast and border
 * faces are the same on all days of the row; for a face to a cell, the first row of that cell with end >= start is
 * found by the binary search of xmhw_object_parts and a cursor moves on from there as the lane walks its days once
 * (rows of a cell are in time order and disjoint); the row under the cursor covers the day iff it has the lane's slot,
 * fits and has started.  The seven addends of a day are formed in registers; one integer atomic without a return
 * value goes out per addend that is not zero, none on a day all of whose faces are shared.  Exact, and the same from
 * run to run.
 * A selected row whose days leave its object's entries or whose cell is outside [0, C) is left out (it neither adds
 * nor covers) and counted in *n_bad_dev (int32; 0 for consistent inputs), as is once a row with a face value outside
 * [XMHW_SHAPE_FACE_FOLDED, C), that face being passed over: nothing outside entries 0..L-1 is ever written, and
 * row_offsets that do not describe the rows read no row outside [0, n).  K other than 4, or n, C, n_slots or L of
 * 2^31 and more: XMHW_ERR_UNSUPPORTED.  Asynchronous on `stream`.                                            */
#define XMHW_SHAPE_CLASSES 3
#define XMHW_SHAPE_OPEN 0
#define XMHW_SHAPE_COAST 1
#define XMHW_SHAPE_BORDER 2
#define XMHW_SHAPE_FACE_COAST (-1)
#define XMHW_SHAPE_FACE_BORDER (-2)
#define XMHW_SHAPE_FACE_FOLDED (-3)
int xmhw_object_shape(const int32_t *start_dev, const int32_t *end_dev, const int32_t *slot_dev,
                      const int32_t *cell_of_row_dev, int64_t n, const int64_t *row_offsets_dev, int64_t C,
                      const int32_t *faces_dev, int32_t K, const int64_t *lq_dev, const int32_t *time_start_dev,
                      const int64_t *offsets_dev, int64_t n_slots, int64_t L, int32_t *edges_dev,
                      int64_t *perimeter_q_dev, int32_t *cells_edge_dev, int32_t *n_bad_dev, void *stream);

/* ---- mhw_track_intensity(): the daily intensity and category series of the objects, ragged ----------- *
 * The one object stage that visits voxels: it joins the series, the climatology and the object partition.  The
 * ragged layout is that of xmhw_object_tracks: selected object i lives from time_start_dev[i] and owns the entries
 * offsets_dev[i] .. offsets_dev[i + 1] - 1, one per day (offsets_dev[n_slots] == L).  A voxel is a step t of a cell c
 * inside a table row (start..end inclusive) whose slot is in [0, n_slots); with x = the sample as float64 (negated
 * when negate != 0) and seas / thresh re-expanded by row_of_t_host (values in [0, D)), its anomaly is a = x - seas,
 * the expression of xmhw_event_stats_*, and it is VALID iff a is not NaN.  Entry offsets[slot] + (t - time_start[slot])
 * receives, over the valid voxels: n_valid += 1, wsum_i += wi[c], isum_q += wi[c] * rint(a * 2^XMHW_TRACK_INTENSITY_BITS),
 * intensity_max = max(a) (compared as float64 through the order-preserving 64-bit key and an integer atomic maximum,
 * -0.0 counted as 0.0; NaN where there is none), and cat_cells[k][.] += 1 for the per-step category of mhw_df(),
 * cats = floor(1 + (x - thresh)/(thresh - seas)): k = 0..3 for cats == 1, == 2, == 3, >= 4 (below the threshold or
 * NaN: none).  A valid voxel with |a| >= 2^7, or infinite, is left out of everything and counted in *n_range_dev; the
 * voxels of a row whose days do not lie within its object's entries are left out and counted in *n_bad_dev (both
 * int64, 0 for consistent inputs): nothing outside entries 0..L-1 is ever written, and with wi <= 2^ib,
 * ib <= 61 - 16 - 7 - bit_length(cells of the grid), |isum_q| stays below 2^61 whatever the data.
 *
 *  1. xmhw_track_intensity_init zeroes the accumulators (n_valid int32[L], wsum_i / isum_q int64[L], intensity_max
 *     [L] used as the key array, cat_cells int32[4][ldcat], ldcat >= L) and both counters.
 *  2. xmhw_track_intensity_accumulate_* handles one slab of n compacted cells: the series ts_dev (T, n) with leading
 *     dimension ld, seas_dev / thresh_dev at the slab's column offset with leading dimension ldc, the slab's n_rows
 *     table rows start_dev / end_dev / slot_dev (int32; the rows of cell c are row_offsets_dev[c] ..
 *     row_offsets_dev[c + 1], relative to the slab's first row, in time order) and wi_dev[n] int64.  It ADDS into
 *     the accumulators: calls for consecutive slabs follow each other on one stream without a read-back.  Lane = cell,
 *     workgroup = 256 cells x XMHW_TRACK_INTENSITY_CHUNK steps; integer atomics without a return value, so the
 *     result is exact and the same whatever the chunks, the slabs and the schedule.
 *  3. xmhw_track_intensity_finish turns the keys into float64.
 * All three are asynchronous on `stream`; nothing is launched for n == 0.  T, n, n_rows, n_slots or L of 2^31 and
 * more: XMHW_ERR_UNSUPPORTED.  xmhw_set_track_intensity_combine (process-wide; tests and measurements): 1 = runs of
 * equal target entries among the lanes of a wave are summed before the atomics (the default), 0 = one set of
 * atomics per voxel.  Same results.                                                                        */
#define XMHW_TRACK_INTENSITY_CHUNK 64
#define XMHW_TRACK_INTENSITY_BITS 16
int xmhw_set_track_intensity_combine(int32_t on);
int xmhw_track_intensity_init(int64_t L, int32_t *n_valid_dev, int64_t *wsum_i_dev, int64_t *isum_q_dev,
                              double *intensity_max_dev, int32_t *cat_cells_dev, int64_t ldcat,
                              int64_t *n_range_dev, int64_t *n_bad_dev, void *stream);
int xmhw_track_intensity_accumulate_f32(const float *ts_dev, int64_t T, int64_t n, int64_t ld,
                                        const double *seas_dev, const double *thresh_dev, int64_t ldc, int64_t D,
                                        const int32_t *row_of_t_host, int32_t negate, const int32_t *start_dev,
                                        const int32_t *end_dev, const int32_t *slot_dev, int64_t n_rows,
                                        const int64_t *row_offsets_dev, const int64_t *wi_dev,
                                        const int32_t *time_start_dev, const int64_t *offsets_dev, int64_t n_slots,
                                        int64_t L, int32_t *n_valid_dev, int64_t *wsum_i_dev, int64_t *isum_q_dev,
                                        double *intensity_max_dev, int32_t *cat_cells_dev, int64_t ldcat,
                                        int64_t *n_range_dev, int64_t *n_bad_dev, void *stream);
int xmhw_track_intensity_accumulate_f64(const double *ts_dev, int64_t T, int64_t n, int64_t ld,
                                        const double *seas_dev, const double *thresh_dev, int64_t ldc, int64_t D,
                                        const int32_t *row_of_t_host, int32_t negate, const int32_t *start_dev,
                                        const int32_t *end_dev, const int32_t *slot_dev, int64_t n_rows,
                                        const int64_t *row_offsets_dev, const int64_t *wi_dev,
                                        const int32_t *time_start_dev, const int64_t *offsets_dev, int64_t n_slots,
                                        int64_t L, int32_t *n_valid_dev, int64_t *wsum_i_dev, int64_t *isum_q_dev,
                                        double *intensity_max_dev, int32_t *cat_cells_dev, int64_t ldcat,
                                        int64_t *n_range_dev, int64_t *n_bad_dev, void *stream);
int xmhw_track_intensity_finish(int64_t L, double *intensity_max_dev, void *stream);

/* ---- mhw_days_by(): per-cell MHW days and intensity by class of time steps --------------------------- *
 * The reduction over TIME that keeps the cell: xmhw_coverage_accumulate_* turned by ninety degrees.  Inputs are those
 * of xmhw_coverage_accumulate_* plus class_of_t_host[T], one int32 class label per step in [-1, K): month, season,
 * year, phase of a climate mode ...; -1 = the step counts nowhere.  A step t of cell c is IN AN EVENT iff detect()
 * labels it (the walk of xmhw_events_from_bits on bits_dev; gap days of joined events included).  With x = the sample
 * as float64 (negated when negate != 0), seas / thresh re-expanded by row_of_t_host:
 *   a   = x - seas                                  (the expression of xmhw_event_stats_*)
 *   cat = floor(1 + (x - thresh)/(thresh - seas))   (the per-step category of mhw_df())
 * For every class k and cell c, over the in-event steps with class_of_t[t] == k:
 *   days[k][0..3][c]      int32    steps with cat == 1, == 2, == 3, >= 4 (moderate, strong, severe, extreme)
 *   days[k][4][c]         int32    all in-event steps (event)
 *   days[k][5][c]         int32    n_valid: in-event steps whose a is not NaN and |a| < 2^7
 *   isum_q[k][c]          int64    sum of rint(a * 2^XMHW_TRACK_INTENSITY_BITS) over the valid steps
 *   intensity_max[k][c]   float64  max a over the valid steps, NaN if there are none
 * An in-event step with a not NaN and |a| >= 2^7 (or infinite) is left out of n_valid, isum_q and intensity_max, is
 * still counted in days[k][0..4][c], and is counted in *n_range_dev (int64; 0 for a series in the units of its
 * climatology).  |isum_q| < 2^31 * 2^23: int64 cannot overflow.  intensity_max goes through the order-preserving 64-bit
 * key and an integer atomic maximum (key 0 = none; -0.0 counts as 0.0).  Cells are the fastest axis of every output:
 * days_dev is int32 [K][XMHW_CLASS_DAYS_CHANNELS][ldo], isum_q_dev int64 [K][ldo], intensity_max_dev float64 [K][ldo],
 * ldo >= C; columns past C are never touched, and a slab addresses its columns by pointer offset, as with the
 * climatologies.  Everything is an integer sum or a maximum: the result is exact and does not depend on the time
 * blocks, the slabs, the launch geometry or the schedule.
 *
 *  1. xmhw_class_days_init zeroes columns 0..C-1 of the accumulators and the counter.
 *  2. xmhw_class_days_accumulate_* handles one slab of C cells and ADDS into the accumulators: calls for consecutive
 *     slabs follow each other on one stream without a read-back.  bits_dev are the words of xmhw_exceed_bits_* for the
 *     same slab (ldb >= C); the in-event bitmap lives in the stream's scratch buffer, as in xmhw_coverage_accumulate_*.
 *     Lane = cell, workgroup = 256 cells x a block of steps; a lane keeps the addends of the current class in
 *     registers and issues integer atomics without a return value when the class changes and at the end of its block.
 *  3. xmhw_class_days_finish turns the keys into float64.
 * All three are asynchronous on `stream`; nothing is launched for C == 0.  K < 1 or K > XMHW_CLASS_DAYS_MAX_CLASSES:
 * XMHW_ERR_UNSUPPORTED, before anything is touched.  T or C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  A label outside
 * [-1, K): XMHW_ERR_INVALID, checked on the host copy before any launch.  xmhw_set_class_days_block (process-wide;
 * tests and measurements): the steps a workgroup takes per block, 0 = automatic.  Same results for every value.   */
#define XMHW_CLASS_DAYS_MAX_CLASSES 1024
#define XMHW_CLASS_DAYS_CHANNELS 6
int xmhw_set_class_days_block(int32_t steps);
int xmhw_class_days_init(int32_t K, int64_t C, int32_t *days_dev, int64_t *isum_q_dev, double *intensity_max_dev,
                         int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_class_days_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *seas_dev,
                                   const double *thresh_dev, int64_t ldc, const int32_t *row_of_t_host,
                                   int32_t negate, const uint64_t *bits_dev, int64_t ldb, int32_t min_duration,
                                   int32_t join_gaps, int32_t max_gap, const int32_t *class_of_t_host, int32_t K,
                                   int32_t *days_dev, int64_t *isum_q_dev, double *intensity_max_dev, int64_t ldo,
                                   int64_t *n_range_dev, void *stream);
int xmhw_class_days_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *seas_dev,
                                   const double *thresh_dev, int64_t ldc, const int32_t *row_of_t_host,
                                   int32_t negate, const uint64_t *bits_dev, int64_t ldb, int32_t min_duration,
                                   int32_t join_gaps, int32_t max_gap, const int32_t *class_of_t_host, int32_t K,
                                   int32_t *days_dev, int64_t *isum_q_dev, double *intensity_max_dev, int64_t ldo,
                                   int64_t *n_range_dev, void *stream);
int xmhw_class_days_finish(int32_t K, int64_t C, double *intensity_max_dev, int64_t ldo, void *stream);

/* ---- mhw_cooccurrence(): per-cell joint event days of two detections, by class of time steps and lag ---- *
 * Compound extremes (joint frequency, likelihood multiplication factor) and verification (the 2x2 contingency table
 * per cell and lead) reduce to the same integers.
 * Two event tables A and B lie on the same time axis of T steps.  For column c and step t, A[t][c] = 1 iff some table
 * row of that cell has start <= t <= end (gap days of joined events included, as detect() stores them).  B is defined
 * the same way.  For a lag l (any int32) the pair (t, l) is VALID iff 0 <= t + l < T.  Then:
 *   Bl[t] = B[t + l] on valid pairs and 0 otherwise.
 *   J[t]  = A[t] & Bl[t], with J[-1] = 0.
 * class_of_t[T] holds int32 labels in [-1, K); -1 counts nowhere.  A pair belongs to the class of t, which is A's step.
 * For every class k, lag index i and column c, summed over the valid pairs with class_of_t[t] == k:
 *   counts[k][i][0][c]   both     A[t] & Bl[t]
 *   counts[k][i][1][c]   a_only   A[t] & ~Bl[t]
 *   counts[k][i][2][c]   b_only   ~A[t] & Bl[t]
 *   counts[k][i][3][c]   onsets   J[t] & ~J[t-1]: the first steps of joint runs
 * The onset test looks at t - 1 whatever the class of t - 1 is.  `neither` is not computed on the device: it is
 * n_pairs[k][i] - both - a_only - b_only, where n_pairs (the number of valid pairs of class k) is computed on the host
 * from the labels and the lag.  All counts are int32 and <= T < 2^31.  A lag with |l| >= T gives zeros everywhere.
 * Everything is an integer sum: the result is exact and does not depend on the time blocks, the lag groups, the slabs
 * or the schedule.
 *
 *  1. xmhw_event_table_bits turns a table into a bitmap, one bit per sample, word-major and cells-minor (the layout of
 *     xmhw_exceed_bits_*): column j is filled from rows offsets[cell[j]] .. offsets[cell[j] + 1] of start_dev / end_dev
 *     (cell may skip and reorder table cells) and written as bits[w * ldb + j], w < W = ceil(T / 64).  Every word of
 *     columns 0..C-1 is written, zero where there is no event: whatever the buffer held before is gone.  The bits at
 *     t >= T of the last word are 0; columns >= C are never touched.  Lane = column: a lane owns its column, so plain
 *     vector stores and no atomics.  The caller guarantees 0 <= start <= end < T and rows of a cell in time order (by
 *     start), as detect() stores them; the kernel relies on it.
 *  2. xmhw_cooccur_init zeroes columns 0..C-1 of the accumulator counts_dev, int32 [K][L][XMHW_COOCCUR_CHANNELS][ldo].
 *  3. xmhw_cooccur_accumulate handles one slab of C cells and ADDS: calls for consecutive slabs follow each other on one
 *     stream without a read-back, and a slab addresses its columns by pointer offset.  a_bits_dev / b_bits_dev are
 *     bitmaps of step 1 (lda, ldb >= C; bits at t >= T zero).  Lane = cell, workgroup = 256 cells x a block of whole
 *     64-step words, grid.z = a group of at most 8 lags; the labels become a per-word segment list on the device, cached
 *     by content; the addends of the current class stay in registers and leave as integer atomics without a return value
 *     when the class changes and at the end of the block.  L = 64 is eight passes over the bitmaps.
 * ldo >= C; columns past C are never touched.  Refusals happen before anything is touched: K < 1,
 * K > XMHW_COOCCUR_MAX_CLASSES, L < 1, L > XMHW_COOCCUR_MAX_LAGS, or T / C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  A
 * label outside [-1, K): XMHW_ERR_INVALID, checked on the host copy.  Nothing is launched for C == 0 or T == 0.  All calls
 * are asynchronous on `stream`.  xmhw_set_cooccur_block (process-wide; tests and measurements): the words a workgroup
 * takes per block, 0 = automatic.  Same results for every value.                                                     */
#define XMHW_COOCCUR_MAX_CLASSES 1024
#define XMHW_COOCCUR_MAX_LAGS    64
#define XMHW_COOCCUR_CHANNELS    4
int xmhw_event_table_bits(const int32_t *start_dev, const int32_t *end_dev, const int64_t *offsets_dev,
                          const int64_t *cell_dev /* [C] */, int64_t C, int64_t T,
                          uint64_t *bits_dev, int64_t ldb, void *stream);
int xmhw_set_cooccur_block(int32_t words);            /* tests and measurements; 0 = automatic */
int xmhw_cooccur_init(int32_t K, int32_t L, int64_t C, int32_t *counts_dev, int64_t ldo, void *stream);
int xmhw_cooccur_accumulate(const uint64_t *a_bits_dev, int64_t lda, const uint64_t *b_bits_dev, int64_t ldb,
                            int64_t T, int64_t C, const int32_t *class_of_t_host, int32_t K,
                            const int32_t *lags_host, int32_t L,
                            int32_t *counts_dev /* [K][L][4][ldo] */, int64_t ldo, void *stream);

/* ---- mhw_displacement(): the thermal displacement of every MHW cell-day (Jacox et al. 2020) ---- *
 * For a grid point in an event on a given day: the distance to the nearest grid point whose sample of that day is no
 * warmer than the event point's own climatology -- how far an organism would have to move to stay at its usual
 * temperature.  The first stage whose cells look at the field around them.
 * The grid is (ny, nx), longitude the fast axis, point p = j * nx + i.  Offsets and distances: a source at (j, i) and a
 * destination at (j', i') have dj = j' - j and di = i' - i, or, on a periodic grid, di = (i' - i) mod nx, minus nx if
 * that exceeds nx / 2 (integer division).  In float64, with the latitudes phi, phi' and dlam = di * dlon in radians:
 *     h       = sin^2((phi' - phi) / 2) + cos phi cos phi' sin^2(dlam / 2), clipped to [0, 1]
 *     dist_m  = rint(1000 radius 2 asin(sqrt(h)))
 *     north_m = rint(1000 radius (phi' - phi))
 *     east_m  = rint(1000 radius cos((phi + phi') / 2) dlam)      (the mid-latitude zonal component)
 * all three functions of (j, dj, di) alone.  The HOST makes, per grid row j, the list of all (dj, di) with
 * 0 <= j + dj < ny, di admissible and dist_m <= rint(1000 max_distance), sorted ascending by (dist_m, dj, di); the first
 * entry is (0, 0).  The lists arrive as CSR: list_off_dev[ny + 1] int64, the packed stream djdi_dev[] (dj << 16 |
 * di & 0xFFFF, both int16) and dist_m_dev[], north_m_dev[], east_m_dev[] int32.  dist_m < 2^25.
 * A SOURCE is a cell-day (c, t) in an event: bit t of column c of bits_dev is set, the bitmap of xmhw_event_table_bits
 * over the C compact (ocean) cells and all T steps.  cell_of_point_dev[ny * nx] int32 maps a grid point to its compact
 * cell (-1: land); basin_dev[ny * nx] int32 (or NULL) holds a basin label per grid point, and a source with a negative
 * label is skipped and counted nowhere.  With x(t, p) = float64(ts[t][p]), negated when `negate`, the target of a source
 * is g = seas_dev[row_of_t[t]][c], and the grid point p = (j + dj, i + di) QUALIFIES iff x(t, p) is not NaN (land is NaN
 * in the uncompacted grid), x(t, p) <= g and, with a basin map, basin[p] == basin[source].  A point outside a
 * non-periodic grid does not qualify; a source with NaN g finds nothing.  The source itself is candidate 0.  The result
 * of a source is the FIRST qualifying entry of its row's list: the minimum of (dist_m, dj, di) over all qualifying
 * points within reach.  Per class k = class_of_t[t] (-1 counts nowhere) and compact cell c:
 *     n_days int32 [K][ldo]    the sources,          n_found int32 [K][ldo]    those that found an entry,
 *     sum_m, sum_north_m, sum_east_m int64 [K][ldo]  the sums of the found entries' dist_m, north_m, east_m,
 *     max_m int32 [K][ldo]     the largest dist_m found, 0 if none,
 * and per call *n_visited_dev int64: the sum over the sources of the list entries that source alone had to look at --
 * the position found plus one, or the whole list length; entries outside the grid included -- defined per source, not
 * per wave, so it does not depend on the schedule.  At most 2^31 steps of less than 2^25 each: int64 cannot overflow.
 * Everything is an integer sum or maximum: the result does not depend on the time blocks, the launch geometry or the
 * schedule.
 *  1. xmhw_displacement_init zeroes columns 0..C-1 of the accumulators and *n_visited_dev.
 *  2. xmhw_displacement_accumulate_* takes the UNCOMPACTED series block ts_dev[nt][ld] (ld >= ny * nx) of the steps
 *     t0 .. t0 + nt - 1, any nt >= 1 with t0 + nt <= T, and ADDS: calls for consecutive blocks follow each other on one
 *     stream without a read-back.  row_of_t_host and class_of_t_host hold all T steps (uploaded once, cached by
 *     content).  Lane = grid point; a wave = 64 consecutive longitudes of one grid row, so it shares one candidate list
 *     and reads 64 consecutive samples per entry; the lanes still searching walk the list together and drop out as they
 *     find; the addends of the current class stay in registers and leave as integer atomics without a return value
 *     when the class changes and at the end of the block.  Every loop is bounded by a list length or the block's steps.
 *     Every index is checked on the device where it is formed, whatever the tables hold.
 * There is no finish call: nothing is kept in an encoded form.  ldo >= C; columns past C are never touched.  Refusals
 * happen before anything is touched: K < 1, K > XMHW_DISPLACEMENT_MAX_CLASSES, T or C of 2^31 and more, ny or nx above
 * XMHW_DISPLACEMENT_MAX_AXIS: XMHW_ERR_UNSUPPORTED.  A label outside [-1, K) or a row outside [0, D): XMHW_ERR_INVALID,
 * checked on the host copies.  Nothing is launched for C == 0.  All calls are asynchronous on `stream`.
 * xmhw_set_displacement_block (process-wide; tests and measurements): the steps a workgroup takes per block,
 * 0 = automatic.  Same results for every value.                                                                      */
#define XMHW_DISPLACEMENT_MAX_CLASSES 1024
#define XMHW_DISPLACEMENT_MAX_AXIS    32767
int xmhw_set_displacement_block(int32_t steps);       /* tests and measurements; 0 = automatic */
int xmhw_displacement_init(int32_t K, int64_t C, int32_t *n_days_dev, int32_t *n_found_dev, int64_t *sum_m_dev,
                           int64_t *sum_north_m_dev, int64_t *sum_east_m_dev, int32_t *max_m_dev, int64_t ldo,
                           int64_t *n_visited_dev, void *stream);
int xmhw_displacement_accumulate_f32(const float *ts_dev, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                     int32_t nx, int32_t periodic, const double *seas_dev, int64_t ldc, int64_t D,
                                     const int32_t *row_of_t_host, int32_t negate, const uint64_t *bits_dev, int64_t ldb,
                                     const int32_t *cell_of_point_dev, int64_t C, const int32_t *basin_dev,
                                     const int64_t *list_off_dev, const int32_t *djdi_dev, const int32_t *dist_m_dev,
                                     const int32_t *north_m_dev, const int32_t *east_m_dev, int64_t n_entries,
                                     const int32_t *class_of_t_host, int32_t K, int32_t *n_days_dev, int32_t *n_found_dev,
                                     int64_t *sum_m_dev, int64_t *sum_north_m_dev, int64_t *sum_east_m_dev,
                                     int32_t *max_m_dev, int64_t ldo, int64_t *n_visited_dev, void *stream);
int xmhw_displacement_accumulate_f64(const double *ts_dev, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                     int32_t nx, int32_t periodic, const double *seas_dev, int64_t ldc, int64_t D,
                                     const int32_t *row_of_t_host, int32_t negate, const uint64_t *bits_dev, int64_t ldb,
                                     const int32_t *cell_of_point_dev, int64_t C, const int32_t *basin_dev,
                                     const int64_t *list_off_dev, const int32_t *djdi_dev, const int32_t *dist_m_dev,
                                     const int32_t *north_m_dev, const int32_t *east_m_dev, int64_t n_entries,
                                     const int32_t *class_of_t_host, int32_t K, int32_t *n_days_dev, int32_t *n_found_dev,
                                     int64_t *sum_m_dev, int64_t *sum_north_m_dev, int64_t *sum_east_m_dev,
                                     int32_t *max_m_dev, int64_t ldo, int64_t *n_visited_dev, void *stream);

/* ---- heat_stress(): accumulated thermal stress (degree heating weeks) and the class sums of the series ---- *
 * The Degree Heating Week of NOAA Coral Reef Watch (Liu et al. 2014; Skirving et al. 2020): how much heat has piled up
 * in a cell over the last W steps.  The first stage with a window along time; one streaming pass over the series, and a
 * second, smaller one for its baseline, the Maximum Monthly Mean, which is made of per-class sums of the plain series.
 *
 * CLASS SUMS.  class_of_t_host[T]: one int32 label per step in [-1, K); -1 = the step counts nowhere.  For every class
 * k and cell c, over the steps of class k, with d = float64(sample) - x0:
 *   n_valid[k][c]         int32    steps whose d is not NaN and |d| < 2^7
 *   sum_q[k][c]           int64    sum of rint(d * 2^XMHW_HEAT_STRESS_BITS) over those steps
 * Any other non-NaN d (|d| >= 2^7 or infinite) is left out and counted in *n_range_dev (int64).  The class mean is
 * x0 + sum_q / n_valid / 2^16; |sum_q| < 2^31 * 2^23: int64 cannot overflow.
 *
 * HEAT STRESS.  base_dev is float64 [D][ldb] with row_of_t_host[T] in [0, D): D = 1 is a constant per cell (the MMM),
 * D = 366 a climatology of threshold().  With x = the sample as float64 and b = base[row_of_t[t]][c], both negated when
 * negate != 0, and h = x - b:
 *   the step is HOT iff h == h, h >= h0 and h < 2^7             (2^-16 <= h0 < 2^7)
 *   q(t) = int64(rint(h * 2^16)) on hot steps, 0 otherwise
 *   S(t) = the sum of q(i) over max(0, t - W + 1) <= i <= t     (1 <= W <= 255: S < 2^31)
 * A step with h >= 2^7 or infinite is not hot and is counted in *n_range_dev, whatever its class (0 for a series in the
 * units of its baseline).  A step of class -1 feeds the window of later steps but is reduced nowhere.  For every class
 * k and cell c, over the steps t with class_of_t[t] == k:
 *   counts[k][0][c]       int32    steps with h not NaN
 *   counts[k][1][c]       int32    hot steps
 *   counts[k][2 + l][c]   int32    steps with S(t) >= level_q_host[l], l < L (int64, strictly ascending); the channels
 *                                  2 + L .. XMHW_HEAT_STRESS_CHANNELS - 1 stay 0
 *   hsum_q[k][c]          int64    sum of q(t): the degree heating days of the class
 *   peak_q[k][c]          int32    max S(t)
 *   peak_t[k][c]          int32    the smallest t that attains peak_q
 * and, whatever the class of the step, for the J snapshot steps at_host[j] (strictly ascending, in [0, T)):
 *   snap_q[j][c]          int32    S(at[j])
 * A class without steps gives peak_q = 0 and peak_t = -1.  The peak is an order-independent 64-bit integer maximum of
 * the key S << 32 | ~t (low word), kept in peak_key_dev (int64 [K][ldo], 0 = no step yet).  Units: level_q =
 * rint(level * unit * 2^16) and DHW = S / (unit * 2^16); Coral Reef Watch's product is W = 84 daily steps, h0 = 1.0,
 * unit = 7, levels 4 and 8.  Everything is an integer sum or an integer maximum: the result is exact and does not depend
 * on the time blocks, the slabs, the launch geometry or the schedule.  Cells are the fastest axis of every output:
 * counts_dev is int32 [K][XMHW_HEAT_STRESS_CHANNELS][ldo], snap_q_dev int32 [J][ldo], the others [K][ldo], ldo >= C;
 * columns past C are never touched, and a slab addresses its columns by pointer offset, as in xmhw_class_days_*.
 *
 *  1. xmhw_class_sums_init / xmhw_heat_stress_init zero columns 0..C-1 of the accumulators and the counter.
 *  2. xmhw_class_sums_accumulate_* / xmhw_heat_stress_accumulate_* handle one slab of C cells and ADDS into the
 *     accumulators; the snapshots are plain stores.  Lane = cell, workgroup = 256 cells x a block of steps; a lane keeps
 *     the addends of the current class in registers and issues integer atomics without a return value when the class
 *     changes and at the end of its block.  A block that starts at t0 > 0 first rebuilds the window from the steps
 *     t0 - W + 1 .. t0 - 1; the step that leaves the window is re-derived from its sample (csrc/kernels_stress.hip).
 *  3. xmhw_heat_stress_finish splits the keys into peak_q_dev and peak_t_dev.
 * All are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: K < 1 or
 * K > XMHW_HEAT_STRESS_MAX_CLASSES, W outside [1, XMHW_HEAT_STRESS_MAX_WINDOW], L > XMHW_HEAT_STRESS_MAX_LEVELS,
 * J > XMHW_HEAT_STRESS_MAX_SNAPSHOTS, T or C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  A bad T, C, D, L, J or leading
 * dimension, h0 outside [2^-16, 2^7) (or NaN; x0 not finite for the class sums), a NULL host table, a label outside
 * [-1, K), a row outside [0, D), levels not strictly ascending, snapshot steps not strictly ascending or outside
 * [0, T): XMHW_ERR_INVALID.  Then nothing is launched for C == 0; then a NULL device buffer is XMHW_ERR_INVALID.
 * xmhw_set_heat_stress_block (process-wide; tests and measurements): the steps a workgroup of either accumulate kernel
 * takes per block, 0 = automatic.  Same results for every value.                                                      */
#define XMHW_HEAT_STRESS_MAX_CLASSES   1024
#define XMHW_HEAT_STRESS_CHANNELS      8
#define XMHW_HEAT_STRESS_MAX_LEVELS    6
#define XMHW_HEAT_STRESS_MAX_SNAPSHOTS 64
#define XMHW_HEAT_STRESS_MAX_WINDOW    255
#define XMHW_HEAT_STRESS_BITS          16
int xmhw_set_heat_stress_block(int32_t steps);        /* tests and measurements; 0 = automatic */
int xmhw_class_sums_init(int32_t K, int64_t C, int32_t *n_valid_dev, int64_t *sum_q_dev, int64_t ldo,
                         int64_t *n_range_dev, void *stream);
int xmhw_class_sums_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, double x0,
                                   const int32_t *class_of_t_host, int32_t K, int32_t *n_valid_dev, int64_t *sum_q_dev,
                                   int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_class_sums_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, double x0,
                                   const int32_t *class_of_t_host, int32_t K, int32_t *n_valid_dev, int64_t *sum_q_dev,
                                   int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_heat_stress_init(int32_t K, int64_t C, int32_t *counts_dev, int64_t *hsum_q_dev, int64_t *peak_key_dev,
                          int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_heat_stress_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                    int64_t ldb, int64_t D, const int32_t *row_of_t_host, int32_t negate, int32_t W,
                                    double h0, const int32_t *class_of_t_host, int32_t K, const int64_t *level_q_host,
                                    int32_t L, const int32_t *at_host, int32_t J, int32_t *counts_dev,
                                    int64_t *hsum_q_dev, int64_t *peak_key_dev, int32_t *snap_q_dev, int64_t ldo,
                                    int64_t *n_range_dev, void *stream);
int xmhw_heat_stress_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                    int64_t ldb, int64_t D, const int32_t *row_of_t_host, int32_t negate, int32_t W,
                                    double h0, const int32_t *class_of_t_host, int32_t K, const int64_t *level_q_host,
                                    int32_t L, const int32_t *at_host, int32_t J, int32_t *counts_dev,
                                    int64_t *hsum_q_dev, int64_t *peak_key_dev, int32_t *snap_q_dev, int64_t ldo,
                                    int64_t *n_range_dev, void *stream);
int xmhw_heat_stress_finish(int32_t K, int64_t C, const int64_t *peak_key_dev, int32_t *peak_q_dev, int32_t *peak_t_dev,
                            int64_t ldo, void *stream);

/* ---- index_regression(): lagged regression and correlation maps of the anomalies on climate indices ---- *
 * What drives the heatwaves of a cell: for every cell the SST anomaly is regressed on an index (Nino-3.4, a basin
 * mean ...) that leads by 0, 30, 60 ... steps, per class of time steps (Holbrook et al. 2019; Sen Gupta et al. 2020).
 * One streaming pass over the series, and the first stage whose per-sample work is a product with a SECOND series: a
 * small matrix product, cells x time against time x predictors, in exact 64-bit integers.
 *
 * ts_dev[T][ld] is the series; base_dev is float64 [D][ldb] with row_of_t_host[T] in [0, D): D = 1 is a constant per
 * cell, D = 366 the `seas` of threshold().  class_of_t_host[T]: one int32 label per step in [-1, K); -1 = the step counts
 * nowhere (and is not read).  zq_host is the predictor table, int32 [T][J], step-major, in fixed point already, with
 * |zq| < 2^XMHW_INDEX_REGRESS_PREDICTOR_BITS (the caller chooses its scale; a lagged predictor is a column of its own).
 * With a = float64(sample) - base[row_of_t[t]][c]:
 *   the step is VALID iff a == a and |a| < 2^7
 *   q(t) = int64(rint(a * 2^XMHW_INDEX_REGRESS_BITS)) on valid steps
 * Any other non-NaN a (|a| >= 2^7 or infinite) of a step with a class is left out everywhere and counted in
 * *n_range_dev (int64).  For every class k and cell c:
 *   n[k][c]        int32   over the valid steps of class k: their count
 *   sa[k][c]       int64   ... the sum of q
 *   saa[k][c]      int64   ... the sum of q^2
 *   n1[k][c]       int32   over the valid steps t >= 1 of class k whose step t - 1 is valid and of class k as well:
 *                          their count
 *   saa1[k][c]     int64   ... the sum of q(t) q(t - 1): with n1, the lag-1 autocorrelation of the cell
 *   saz[k][j][c]   int64   over the valid steps of class k: the sum of q(t) zq[t][j]
 *   mz[k][j][c]    int64   over the steps of class k that are NOT valid (NaN or out of range): the sum of zq[t][j]
 *   mzz[k][j][c]   int64   ... the sum of zq[t][j]^2
 * mz and mzz are deficits: the caller computes the sums of zq and zq^2 over all steps of a class once, and a cell's own
 * sums over its valid steps are those minus its deficits.  T < 2^17 keeps every sum below 2^63 (2^17 * 2^23 * 2^23).
 * Everything is an integer sum: the result is exact and does not depend on the time blocks, the slabs, the launch
 * geometry or the schedule.  Cells are the fastest axis of every output: saz, mz and mzz are [K][J][ldo], the others
 * [K][ldo], ldo >= C; columns past C are never touched, and a slab addresses its columns by pointer offset, as in
 * xmhw_heat_stress_*.
 *
 *  1. xmhw_index_regress_init zeroes columns 0..C-1 of the accumulators and the counter.
 *  2. xmhw_index_regress_accumulate_* handles one slab of C cells and ADDS into the accumulators.  Lane = cell,
 *     workgroup = 256 cells x a block of steps; a lane keeps the addends of the current class in registers (one 64-bit
 *     multiply-add per predictor and step) and issues integer atomics without a return value when the class changes and
 *     at the end of its block; a step that is not valid issues its deficits directly.  A block that starts at t0 > 0
 *     reads step t0 - 1 once for the lag-1 pair (csrc/kernels_regress.hip).
 * Both are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: K < 1 or
 * K > XMHW_INDEX_REGRESS_MAX_CLASSES, J < 1 or J > XMHW_INDEX_REGRESS_MAX_PREDICTORS, T of 2^17 and more, C of 2^31 and
 * more: XMHW_ERR_UNSUPPORTED.  A bad T, C, D or leading dimension, a NULL host table, a label outside [-1, K), a row
 * outside [0, D), a predictor outside (-2^23, 2^23): XMHW_ERR_INVALID.  Then nothing is launched for C == 0; then a NULL
 * device buffer is XMHW_ERR_INVALID.
 * xmhw_set_index_regress_block (process-wide; tests and measurements): the steps a workgroup takes per block,
 * 0 = automatic.  Same results for every value.                                                                      */
#define XMHW_INDEX_REGRESS_MAX_PREDICTORS 32
#define XMHW_INDEX_REGRESS_MAX_CLASSES    64
#define XMHW_INDEX_REGRESS_MAX_STEPS      131072     /* T below it */
#define XMHW_INDEX_REGRESS_BITS           16
#define XMHW_INDEX_REGRESS_RANGE_BITS     7
#define XMHW_INDEX_REGRESS_PREDICTOR_BITS 23
int xmhw_set_index_regress_block(int32_t steps);      /* tests and measurements; 0 = automatic */
int xmhw_index_regress_init(int32_t K, int32_t J, int64_t C, int32_t *n_dev, int64_t *sa_dev, int64_t *saa_dev,
                            int32_t *n1_dev, int64_t *saa1_dev, int64_t *saz_dev, int64_t *mz_dev, int64_t *mzz_dev,
                            int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_index_regress_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                      int64_t ldb, int64_t D, const int32_t *row_of_t_host, const int32_t *class_of_t_host,
                                      int32_t K, const int32_t *zq_host, int32_t J, int32_t *n_dev, int64_t *sa_dev,
                                      int64_t *saa_dev, int32_t *n1_dev, int64_t *saa1_dev, int64_t *saz_dev,
                                      int64_t *mz_dev, int64_t *mzz_dev, int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_index_regress_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                      int64_t ldb, int64_t D, const int32_t *row_of_t_host, const int32_t *class_of_t_host,
                                      int32_t K, const int32_t *zq_host, int32_t J, int32_t *n_dev, int64_t *sa_dev,
                                      int64_t *saa_dev, int32_t *n1_dev, int64_t *saa1_dev, int64_t *saz_dev,
                                      int64_t *mz_dev, int64_t *mzz_dev, int64_t ldo, int64_t *n_range_dev, void *stream);

/* ---- mhw_composite(): event-centred composites (superposed epoch analysis) of a field, per cell ---- *
 * What a field looks like 30 days before every heatwave onset of a cell, at the peak, 20 days after the end (Holbrook et
 * al. 2019; Sen Gupta et al. 2020): the first stage whose per-sample work is keyed by the distance to an event of the
 * lane's own cell.
 *
 * ts_dev[T][ld] is the series (the SST anomaly's series itself, or wind stress, heat flux, mixed-layer depth on the same
 * cells); base_dev is float64 [Dr][ldb] with row_of_t_host[T] in [0, Dr): Dr = 1 is a constant per cell, read once.
 * anchor_bits_dev is the anchor bitmap in the layout of xmhw_event_table_bits (bits[w * lda + c], bits at t >= T zero;
 * table rows with start == end make it the anchor rasteriser).  class_of_t_host[T]: one int32 label per step in [-1, K).
 * before >= 0 and after >= 0 with D = before + after + 1 <= XMHW_COMPOSITE_MAX_OFFSETS; shift in
 * [0, XMHW_COMPOSITE_MAX_SHIFT].  For every cell c, every anchor step s of c with k = class_of_t[s] >= 0 and every offset
 * d in [-before, after] with 0 <= s + d < T:
 *   a = (float64(ts[s + d][c]) - base[row_of_t[s + d]][c]) * 2^-shift       (the scaling is exact)
 *   a NaN adds nothing; |a| >= 2^7 or infinite adds 1 to *n_range_dev (int64); otherwise
 *   q = int64(rint(a * 2^XMHW_COMPOSITE_BITS)) and, with i = d + before,
 *   n[k][i][c] += 1 (int32), s[k][i][c] += q (int64), ss[k][i][c] += q^2 (int64).
 * The class is that of the ANCHOR step, not of the sample: an event belongs to the season or ENSO phase of its onset.
 * Anchors of class -1 count nowhere, n_range included.  shift exists because the 2^7 range is an SST range: heat flux in
 * W m^-2 needs shift = 4 or so, and the resolution becomes 2^(shift - 16).  T < 2^17, |q| <= 2^23, q^2 <= 2^46 and at most
 * T anchors per entry: every sum stays inside 64 bits.  Everything is an integer sum: the result is exact and does not
 * depend on the time blocks, the slabs, the launch geometry or the schedule.  The outputs are [K][D][ldo], ldo >= C;
 * columns past C are never touched, and a slab addresses its columns by pointer offset.
 *
 *  1. xmhw_composite_init zeroes columns 0..C-1 of the accumulators and the counter.
 *  2. xmhw_composite_accumulate_* handles one slab of C cells and ADDS into the accumulators.  Lane = cell, workgroup =
 *     256 cells x a block of steps; a lane carries a window of D bits (bit i: an anchor at step t + before - i), a step
 *     on which no lane of a wave has a bit set requests no sample, and every set bit issues its three integer atomics
 *     without a return value.  A block builds its window from bitmap words alone (csrc/kernels_composite.hip).
 * Both are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: before or after < 0, K < 1 or
 * K > XMHW_COMPOSITE_MAX_CLASSES, D > XMHW_COMPOSITE_MAX_OFFSETS, shift outside [0, XMHW_COMPOSITE_MAX_SHIFT], T of 2^17
 * and more, C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  A bad T, C, Dr or leading dimension, a NULL host table, a label
 * outside [-1, K), a row outside [0, Dr): XMHW_ERR_INVALID.  Then nothing is launched for C == 0 or T == 0; then a NULL
 * device buffer is XMHW_ERR_INVALID.
 * xmhw_set_composite_block (process-wide; tests and measurements): the steps a workgroup takes per block, 0 = automatic.
 * Same results for every value.                                                                                       */
#define XMHW_COMPOSITE_MAX_OFFSETS 128
#define XMHW_COMPOSITE_MAX_CLASSES 64
#define XMHW_COMPOSITE_MAX_STEPS   131072            /* T below it */
#define XMHW_COMPOSITE_BITS        16
#define XMHW_COMPOSITE_RANGE_BITS  7
#define XMHW_COMPOSITE_MAX_SHIFT   24
int xmhw_set_composite_block(int32_t steps);          /* tests and measurements; 0 = automatic */
int xmhw_composite_init(int32_t K, int32_t D, int64_t C, int32_t *n_dev, int64_t *s_dev, int64_t *ss_dev, int64_t ldo,
                        int64_t *n_range_dev, void *stream);
int xmhw_composite_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev, int64_t ldb,
                                  int64_t Dr, const int32_t *row_of_t_host, int32_t shift, const uint64_t *anchor_bits_dev,
                                  int64_t lda, const int32_t *class_of_t_host, int32_t K, int32_t before, int32_t after,
                                  int32_t *n_dev, int64_t *s_dev, int64_t *ss_dev, int64_t ldo, int64_t *n_range_dev,
                                  void *stream);
int xmhw_composite_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                  int64_t ldb, int64_t Dr, const int32_t *row_of_t_host, int32_t shift,
                                  const uint64_t *anchor_bits_dev, int64_t lda, const int32_t *class_of_t_host, int32_t K,
                                  int32_t before, int32_t after, int32_t *n_dev, int64_t *s_dev, int64_t *ss_dev,
                                  int64_t ldo, int64_t *n_range_dev, void *stream);

/* ---- lag_correlation(): per-cell lagged auto- and cross-correlation ---- *
 * The memory of the anomaly of a cell (autocorrelation function, e-folding time, integral time scale, effective sample
 * size: Holbrook et al. 2019; Jacox et al. 2022) and the lagged correlation of two fields in the same cell (net heat flux,
 * wind stress or mixed-layer depth against the SST anomaly): the first stage that multiplies a sample by the lane's own
 * past, or by the past of a second resident series.
 *
 * x_dev[T][ldx] and y_dev[T][ldy] are two series of the same float type; y_dev may be the very buffer of x_dev
 * (autocorrelation), with the same bits as a separate copy.  base_x_dev[Dr][ldbx] and base_y_dev[Dr][ldby] are float64 with
 * ONE row_of_t_host[T] in [0, Dr): Dr = 1 is a constant per cell, read once.  shift_x, shift_y in
 * [0, XMHW_LAG_CORR_MAX_SHIFT]; class_of_t_host[T]: one int32 label per step in [-1, K), K <= XMHW_LAG_CORR_MAX_CLASSES;
 * max_lag = L in [0, XMHW_LAG_CORR_MAX_LAG]; T < 2^17, C < 2^31.
 *   ax(t) = (float64(x[t][c]) - base_x[row_of_t[t]][c]) * 2^-shift_x, likewise ay       (the scaling is exact)
 *   a value is VALID iff it is not NaN and |a| < 2^XMHW_LAG_CORR_RANGE_BITS; q = int64(rint(a * 2^XMHW_LAG_CORR_BITS)).
 * For every cell c, every step t with k = class_of_t[t] >= 0, every lag l in [0, L] with t - l >= 0, and ax(t) and
 * ay(t - l) both valid:
 *   n  [k][l][c] += 1 (int32)        sx [k][l][c] += qx(t)          sy [k][l][c] += qy(t - l)
 *   sxx[k][l][c] += qx(t)^2          syy[k][l][c] += qy(t - l)^2    sxy[k][l][c] += qx(t) qy(t - l)      (all int64)
 * The class of a pair is that of its LATER step; the earlier step may be of any class, -1 included.  All six sums run
 * over the valid pairs alone (pairwise deletion), so Pearson's r of every lag is a true correlation.  |q| <= 2^23,
 * products <= 2^46, fewer than 2^17 pairs per entry: everything stays inside 64 bits.  n_range_dev[2] (int64): [0] counts
 * the steps of class >= 0 at which ax is not NaN and out of range, [1] the steps of any class at which ay is; each step
 * once, whatever the blocks.  x is not read on steps of class -1.  Everything is an integer sum: the result is exact and
 * does not depend on the time blocks, the slabs, the launch geometry or the schedule.  The outputs are [K][L + 1][ldo],
 * ldo >= C; columns past C are never touched, and a slab addresses its columns by pointer offset.
 *
 *  1. xmhw_lag_corr_init zeroes columns 0..C-1 of the accumulators and the two counters.
 *  2. xmhw_lag_corr_accumulate_* handles one slab of C cells and ADDS into the accumulators: two calls on disjoint column
 *     ranges equal one.  Lane = cell, workgroup = 256 cells x a block of steps x a group of 8 or 16 lags; qy of the last steps
 *     in an LDS ring of 16 / 32 / 64 slots per lane, their validity in a 64-bit mask; a block rebuilds both from the
 *     max_lag steps before it (csrc/kernels_lagcorr.hip, csrc/lag_ring.h).
 * Both are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: K < 1 or
 * K > XMHW_LAG_CORR_MAX_CLASSES, max_lag outside [0, XMHW_LAG_CORR_MAX_LAG], a shift outside [0, XMHW_LAG_CORR_MAX_SHIFT],
 * T of 2^17 and more, C of 2^31 and more: XMHW_ERR_UNSUPPORTED.  A bad T, C, Dr or leading dimension, a NULL host table, a
 * label outside [-1, K), a row outside [0, Dr): XMHW_ERR_INVALID.  Then nothing is launched for C == 0 or T == 0; then a
 * NULL device buffer is XMHW_ERR_INVALID.
 * xmhw_set_lag_corr_block (process-wide; tests and measurements): the steps a workgroup takes per block, 0 = automatic,
 * a negative value is XMHW_ERR_INVALID.  Same results for every value.                                               */
#define XMHW_LAG_CORR_MAX_LAG      63
#define XMHW_LAG_CORR_MAX_CLASSES  64
#define XMHW_LAG_CORR_MAX_STEPS    131072            /* T below it */
#define XMHW_LAG_CORR_BITS         16
#define XMHW_LAG_CORR_RANGE_BITS   7
#define XMHW_LAG_CORR_MAX_SHIFT    24
int xmhw_set_lag_corr_block(int32_t steps);           /* tests and measurements; 0 = automatic */
int xmhw_lag_corr_init(int32_t K, int32_t max_lag, int64_t C, int32_t *n_dev, int64_t *sx_dev, int64_t *sy_dev,
                       int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_lag_corr_accumulate_f32(const float *x_dev, int64_t ldx, const float *y_dev, int64_t ldy, int64_t T, int64_t C,
                                 const double *base_x_dev, int64_t ldbx, const double *base_y_dev, int64_t ldby, int64_t Dr,
                                 const int32_t *row_of_t_host, int32_t shift_x, int32_t shift_y,
                                 const int32_t *class_of_t_host, int32_t K, int32_t max_lag, int32_t *n_dev, int64_t *sx_dev,
                                 int64_t *sy_dev, int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo,
                                 int64_t *n_range_dev, void *stream);
int xmhw_lag_corr_accumulate_f64(const double *x_dev, int64_t ldx, const double *y_dev, int64_t ldy, int64_t T, int64_t C,
                                 const double *base_x_dev, int64_t ldbx, const double *base_y_dev, int64_t ldby, int64_t Dr,
                                 const int32_t *row_of_t_host, int32_t shift_x, int32_t shift_y,
                                 const int32_t *class_of_t_host, int32_t K, int32_t max_lag, int32_t *n_dev, int64_t *sx_dev,
                                 int64_t *sy_dev, int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo,
                                 int64_t *n_range_dev, void *stream);

/* ---- anomaly_distribution(): per-cell histograms, quantiles and moments of the anomaly ---- *
 * What the distribution of the anomaly of a cell looks like, per class of time steps: skewness and kurtosis (why heatwaves
 * and cold spells of one cell are not mirror images: Sura & Sardeshmukh 2008; the check on every Gaussian p-value),
 * quantile maps that are not the day-of-year threshold, exceedance probabilities at levels of the user's choosing.  The
 * first stage whose accumulator's address is the sample: a per-lane histogram in LDS, and sums 128 bits wide.
 *
 * ts_dev[T][ld] is a series of float32 / float64; base_dev[Dr][ldb] is float64 with row_of_t_host[T] in [0, Dr): Dr = 1 is a
 * constant per cell, read once.  shift in [0, XMHW_DISTRIBUTION_MAX_SHIFT]; class_of_t_host[T]: one int32 label per step in
 * [-1, K), K <= XMHW_DISTRIBUTION_MAX_CLASSES, -1 counts nowhere (the step is not read); T < 2^17, C < 2^31.
 *   d(t) = (float64(ts[t][c]) - base[row_of_t[t]][c]) * 2^-shift                        (the scaling is exact)
 *   NaN is no sample; |d| >= 2^XMHW_DISTRIBUTION_RANGE_BITS (infinities included) is left out and counted in *n_range_dev;
 *   otherwise the step is VALID and q = int64(rint(d * 2^XMHW_DISTRIBUTION_BITS)), |q| <= 2^23.
 * The bins are lo_q (|lo_q| <= 2^23), width_q >= 1 and B in [1, XMHW_DISTRIBUTION_MAX_BINS]: the bin of q is
 * b = floor((q - lo_q) / width_q), exactly; b < 0 counts in the UNDER row (row 0), b >= B in the OVER row (row B + 1),
 * anything else in row 1 + b.  For every class k and cell c, over the valid steps of class k, exact integers:
 *   hist[k][0 .. B + 1][c]  int32   the counts per row
 *   n   [k][c]              int32   the valid steps (the sum of the rows)
 *   s1, s2 [k][c]           int64   the sums of q and q^2 (fewer than 2^17 steps of at most 2^46)
 *   s3, s4 [k][0 .. 1][c]           the sums of q^3 and q^4 as 128-bit two's-complement integers: [k][0] the low words
 *                                   (to be read as uint64), [k][1] the high words (int64)
 *   kmax, kmin [k][c]       uint64  the order-preserving keys of the largest d and of the largest -d (0: none); after
 *                                   xmhw_distribution_finish float64: the largest and the smallest d, NaN for none
 * All outputs have the cells as their fastest axis with leading dimension ldo >= C; columns past C are never touched, and
 * a slab addresses its columns by pointer offset.  Everything is an integer sum, an integer maximum or a function of
 * those: the result does not depend on the time blocks, the slabs, the launch geometry or the schedule.
 *
 *  1. xmhw_distribution_init zeroes columns 0..C-1 of the ten accumulators and the counter.
 *  2. xmhw_distribution_accumulate_* handles one slab of C cells and ADDS into the accumulators: two calls on disjoint
 *     column ranges equal one.  Lane = cell, workgroup = 256 cells x a block of steps; the histogram of a lane is a column
 *     of 16-bit halves in LDS (32 / 64 / 128 KB for B <= 64 / 128 / 256), flushed by integer atomics when the class changes,
 *     at the end of the block and after 65,535 steps of a run (csrc/kernels_distribution.hip, csrc/hist_bin.h,
 *     csrc/wide_sum.h).
 *  3. xmhw_distribution_finish, once per column after the last slab, works from the device-resident histogram: the keys
 *     become float64, and for P <= XMHW_DISTRIBUTION_MAX_QUANTILES probabilities p_q_host[j] = rint(p * 2^32) in
 *     [0, 2^32], with the rank r = max(1, ceil(p_q * n / 2^32)) in 64-bit integers,
 *       qbin  [k][j][c] int32: the bin that holds the r-th smallest valid sample; -1 = UNDER, B = OVER, INT32_MIN: n == 0
 *       qbelow[k][j][c] int32: the valid samples in rows strictly below that row (0 for n == 0)
 *       qcount[k][j][c] int32: the valid samples in that row (0 for n == 0): what a quantile inside the bin needs
 *     and for L <= XMHW_DISTRIBUTION_MAX_LEVELS edges edge_host[l] in [0, B]
 *       n_at_least[k][l][c] int32: the valid samples with b >= edge[l] (edge 0: everything but UNDER; edge B: OVER).
 * All three are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: K < 1 or
 * K > XMHW_DISTRIBUTION_MAX_CLASSES, B < 1 or B > XMHW_DISTRIBUTION_MAX_BINS, T of 2^17 and more, C of 2^31 and more, then
 * (accumulate) width_q < 1, lo_q outside [-2^23, 2^23], a shift outside [0, XMHW_DISTRIBUTION_MAX_SHIFT], (finish) P or L
 * outside their range: XMHW_ERR_UNSUPPORTED.  A bad T, C, Dr or leading dimension, a NULL host table, a label outside
 * [-1, K), a row outside [0, Dr), a p_q above 2^32, an edge outside [0, B]: XMHW_ERR_INVALID.  Then nothing is launched for
 * C == 0 (or T == 0); then a NULL device buffer is XMHW_ERR_INVALID (qbin, qbelow and qcount may be NULL for P == 0, n_at_least for
 * L == 0).
 * xmhw_set_distribution_block (process-wide; tests and measurements): the steps a workgroup takes per block, 0 = automatic,
 * a negative value is XMHW_ERR_INVALID.  Same results for every value.                                               */
#define XMHW_DISTRIBUTION_MAX_BINS       256
#define XMHW_DISTRIBUTION_MAX_CLASSES    64
#define XMHW_DISTRIBUTION_MAX_QUANTILES  16
#define XMHW_DISTRIBUTION_MAX_LEVELS     8
#define XMHW_DISTRIBUTION_MAX_STEPS      (1 << 17)   /* T below it */
#define XMHW_DISTRIBUTION_BITS           16
#define XMHW_DISTRIBUTION_RANGE_BITS     7
#define XMHW_DISTRIBUTION_MAX_SHIFT      24
int xmhw_set_distribution_block(int32_t steps);       /* tests and measurements; 0 = automatic */
int xmhw_distribution_init(int32_t K, int32_t B, int64_t C, int32_t *hist_dev, int32_t *n_dev, int64_t *s1_dev, int64_t *s2_dev,
                           int64_t *s3_dev, int64_t *s4_dev, uint64_t *kmin_dev, uint64_t *kmax_dev, int64_t ldo,
                           int64_t *n_range_dev, void *stream);
int xmhw_distribution_accumulate_f32(const float *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev, int64_t ldb,
                                     int64_t Dr, const int32_t *row_of_t_host, int32_t shift, const int32_t *class_of_t_host,
                                     int32_t K, int64_t lo_q, int32_t width_q, int32_t B, int32_t *hist_dev, int32_t *n_dev,
                                     int64_t *s1_dev, int64_t *s2_dev, int64_t *s3_dev, int64_t *s4_dev, uint64_t *kmin_dev,
                                     uint64_t *kmax_dev, int64_t ldo, int64_t *n_range_dev, void *stream);
int xmhw_distribution_accumulate_f64(const double *ts_dev, int64_t T, int64_t C, int64_t ld, const double *base_dev,
                                     int64_t ldb, int64_t Dr, const int32_t *row_of_t_host, int32_t shift,
                                     const int32_t *class_of_t_host, int32_t K, int64_t lo_q, int32_t width_q, int32_t B,
                                     int32_t *hist_dev, int32_t *n_dev, int64_t *s1_dev, int64_t *s2_dev, int64_t *s3_dev,
                                     int64_t *s4_dev, uint64_t *kmin_dev, uint64_t *kmax_dev, int64_t ldo,
                                     int64_t *n_range_dev, void *stream);
int xmhw_distribution_finish(int32_t K, int32_t B, int64_t C, const int32_t *hist_dev, const int32_t *n_dev, double *kmin_dev,
                             double *kmax_dev, const uint64_t *p_q_host, int32_t P, const int32_t *edge_host, int32_t L,
                             int32_t *qbin_dev, int32_t *qbelow_dev, int32_t *qcount_dev, int32_t *n_at_least_dev, int64_t ldo,
                             void *stream);

/* ---- spatial_correlation(): per-cell correlation with grid neighbours ---- *
 * The spatial correlation function of the anomaly and its decorrelation length: how large heatwaves are, the spatial
 * counterpart of the e-folding time, and the input to every field-significance statement (the effective number of
 * independent cells of a map).  The first stage whose per-sample work is a product with the samples of OTHER grid points at
 * the same step: a stencil over a tile with a halo in LDS.
 *
 * ts_dev[nt][ld] is a block of steps t0 .. t0 + nt - 1 of the UNCOMPACTED series on the ny x nx grid, float32 or float64,
 * ld >= ny * nx, land NaN; point p = j * nx + i, longitude the fast axis.  base_dev[Dr][ldb] is float64 on the same grid
 * (ldb >= ny * nx) with row_of_t_host[T] in [0, Dr): Dr = 1 is a constant per point, read once.  shift in
 * [0, XMHW_SPATIAL_CORR_MAX_SHIFT]; class_of_t_host[T]: one int32 label per step in [-1, K), K <=
 * XMHW_SPATIAL_CORR_MAX_CLASSES; periodic != 0: longitude wraps; T < 2^17; ny, nx <= XMHW_SPATIAL_CORR_MAX_AXIS.
 * offsets_host[D][2] holds D offsets (dj, di) as int32 pairs, 1 <= D <= XMHW_SPATIAL_CORR_MAX_OFFSETS, |dj|, |di| <=
 * XMHW_SPATIAL_CORR_REACH; duplicates and (0, 0) are allowed; with periodic, an offset with |di| >= nx is XMHW_ERR_INVALID.
 *   a(t, p) = (float64(ts[t][p]) - base[row_of_t[t]][p]) * 2^-shift                     (the scaling is exact)
 *   a sample is VALID iff a is not NaN and |a| < 2^XMHW_SPATIAL_CORR_RANGE_BITS; q = int64(rint(a * 2^XMHW_SPATIAL_CORR_BITS)).
 * For every grid point p = (j, i), every step t of the block with k = class_of_t[t] >= 0 and every offset e = (dj, di),
 * the partner is p' = (j + dj, i + di), i + di taken mod nx when periodic.  The pair is valid iff p' lies in the grid and
 * a(t, p) and a(t, p') are both valid; for a valid pair, into the outputs [K][D][ldo], ldo >= ny * nx:
 *   n  [k][e][p] += 1 (int32)        sx [k][e][p] += q(p)           sy [k][e][p] += q(p')
 *   sxx[k][e][p] += q(p)^2           syy[k][e][p] += q(p')^2        sxy[k][e][p] += q(p) q(p')           (all int64)
 * All six sums run over the valid pairs alone (pairwise deletion, as in lag_correlation()).  Land points keep n = 0;
 * columns past ny * nx are never touched; steps of class -1 are not read.  *n_range_dev (int64) counts the (t, p) of class
 * >= 0 whose a is not NaN and out of range: each once, by its own point, whatever the blocks, tiles and halos; such a
 * sample is no partner either.  |q| <= 2^23, products <= 2^46, fewer than 2^17 pairs per entry: everything stays inside 64
 * bits.  Everything is an integer sum: the result is exact and does not depend on the time blocks, the tile geometry, the
 * offset grouping or the schedule.
 *
 *  1. xmhw_spatial_corr_init zeroes columns 0 .. ny * nx - 1 of the accumulators and the counter.
 *  2. xmhw_spatial_corr_accumulate_* ADDS the block: consecutive blocks follow each other on one stream without a
 *     read-back.  A workgroup owns a tile of 8 grid rows x 64 longitudes, walks a block of steps and takes a group of 8 or
 *     16 offsets; per step it converts the tile and the halo the group's offsets reach once into LDS, and every lane reads
 *     one dword per offset (csrc/kernels_spatialcorr.hip, csrc/halo_tile.h).
 * Both are asynchronous on `stream`.  Refusals, in this order and before the first HIP call: K < 1 or
 * K > XMHW_SPATIAL_CORR_MAX_CLASSES, D < 1 or D > XMHW_SPATIAL_CORR_MAX_OFFSETS, a shift outside
 * [0, XMHW_SPATIAL_CORR_MAX_SHIFT], T of 2^17 and more, a grid axis above XMHW_SPATIAL_CORR_MAX_AXIS, an offset (of a table
 * that is not NULL) beyond XMHW_SPATIAL_CORR_REACH: XMHW_ERR_UNSUPPORTED.  A negative ny or nx, a bad T, t0 or nt (0 <= t0,
 * 0 <= nt <= T - t0), a bad leading dimension or Dr, a NULL host table (offsets always; the labels and rows for T > 0), an
 * offset with |di| >= nx on a periodic grid, a label outside [-1, K), a row outside [0, Dr): XMHW_ERR_INVALID.  Then
 * nothing is launched for nt == 0 or ny * nx == 0; then a NULL device buffer is XMHW_ERR_INVALID.
 * xmhw_set_spatial_corr_block (process-wide; tests and measurements): the steps a workgroup takes per block, 0 = automatic,
 * a negative value is XMHW_ERR_INVALID.  xmhw_set_spatial_corr_tile (likewise): the grid rows of a tile, 4 or 8, 0 = the
 * default (8).  Same results for every value of either.                                                            */
#define XMHW_SPATIAL_CORR_MAX_OFFSETS 64
#define XMHW_SPATIAL_CORR_REACH       32
#define XMHW_SPATIAL_CORR_MAX_CLASSES 64
#define XMHW_SPATIAL_CORR_MAX_STEPS   131072         /* T below it */
#define XMHW_SPATIAL_CORR_MAX_AXIS    32767
#define XMHW_SPATIAL_CORR_BITS        16
#define XMHW_SPATIAL_CORR_RANGE_BITS  7
#define XMHW_SPATIAL_CORR_MAX_SHIFT   24
int xmhw_set_spatial_corr_block(int32_t steps);       /* tests and measurements; 0 = automatic */
int xmhw_set_spatial_corr_tile(int32_t rows);         /* tests and measurements; 0 = the default */
int xmhw_spatial_corr_init(int32_t K, int32_t D, int32_t ny, int32_t nx, int32_t *n_dev, int64_t *sx_dev, int64_t *sy_dev,
                           int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo, int64_t *n_range_dev,
                           void *stream);
int xmhw_spatial_corr_accumulate_f32(const float *ts_dev, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                     int32_t nx, int32_t periodic, const double *base_dev, int64_t ldb, int64_t Dr,
                                     const int32_t *row_of_t_host, int32_t shift, const int32_t *class_of_t_host, int32_t K,
                                     const int32_t *offsets_host, int32_t D, int32_t *n_dev, int64_t *sx_dev, int64_t *sy_dev,
                                     int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo, int64_t *n_range_dev,
                                     void *stream);
int xmhw_spatial_corr_accumulate_f64(const double *ts_dev, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny,
                                     int32_t nx, int32_t periodic, const double *base_dev, int64_t ldb, int64_t Dr,
                                     const int32_t *row_of_t_host, int32_t shift, const int32_t *class_of_t_host, int32_t K,
                                     const int32_t *offsets_host, int32_t D, int32_t *n_dev, int64_t *sx_dev, int64_t *sy_dev,
                                     int64_t *sxx_dev, int64_t *syy_dev, int64_t *sxy_dev, int64_t ldo, int64_t *n_range_dev,
                                     void *stream);

/* ---- coarsen(): weighted block means in space and time ---- *
 * The front-end stage: daily series to pentad or monthly means, a fine tile to the grid of a climatology, the grid under a
 * reach or a lag range that the analysis stages cap.  Every sample is read once; the output is fy * fx * len times smaller.
 *
 * Inputs.  ts_dev[nt][ld] is the fine series x[t][j][i], UNCOMPACTED on the ny x nx grid, longitude the fast axis, float32
 * or float64, ld >= ny * nx, NaN = no sample.  wi_dev[ny * nx] int32 weights, 0 <= wi <= 2^24 (not checked: they live on
 * the device).  Spatial factors fy, fx >= 1.  The coarse grid is ncy x ncx with ncy <= ceil(ny / fy), ncx <= ceil(nx / fx):
 * the caller chooses floor or ceil (or fewer); a block that hangs over the grid holds only its in-grid points.
 * win_host[ns + 1] int32, relative to the first row passed, strictly increasing, win[0] >= 0, win[ns] <= nt: window s covers
 * rows win[s] .. win[s + 1] - 1; rows in no window are not read.
 *
 * Sums.  For the coarse entry (s, J, I), over the in-grid fine samples of block x window that have wi > 0 and are not NaN:
 *   xq = rint(((double)x - x0) * 2^XMHW_REGION_SERIES_BITS)     (the fixed point of region_series(), in float64 as written)
 *   a sample with |x - x0| >= 2^7, or infinite, is left out of all sums and counted in *n_range_dev (int64, ADDED to)
 *   n += 1, wsum += wi, xsum += wi * xq                          (exact integers)
 * W = the sum of wi over the in-grid points of the block, land included; len = the window's length.
 *
 * Validity.  The entry is valid iff n >= 1 and wsum * 65536 >= a * len * W; a is an integer in [0, 65536], the least
 * covered share in 65536ths; equality counts as valid.
 *
 * Output.  out_dev[s][J * ncx + I] = x0 + ((double)xsum / (double)wsum) / 65536.0, in float64 exactly as written, rounded
 * once to the sample type; NaN for an invalid entry.  out_dev[ns][ldo] (ldo >= ncy * ncx) is WRITTEN, not added to; columns
 * past ncy * ncx are never touched.  wsum_dev (int64 [ns][ldo]) and n_dev (int32 [ns][ldo]) are optional: NULL = not written.
 *
 * Cap and overflow.  fy * fx * (the longest window) <= XMHW_COARSEN_MAX_VOLUME = 4096, else XMHW_ERR_UNSUPPORTED.  With the
 * cap |xsum| <= 2^12 * 2^24 * 2^23 = 2^59, wsum * 65536 < 2^52 and a * len * W <= 2^52.  The finish is two integer-to-double
 * conversions, one correctly rounded division, an exact scaling and one add (the build uses -ffp-contract=off): numpy
 * reproduces every bit.  The result does not depend on launch geometry, window chunks, time blocks or load widths.
 *
 * Refusals, in this order and before the first HIP call: a volume above the cap, ny * nx of 2^31 and more:
 * XMHW_ERR_UNSUPPORTED.  A negative nt, ny or nx, ld < ny * nx, a factor below 1, ncy or ncx negative or above ceil, ldo <
 * ncy * ncx, a negative ns, a NULL win_host with ns > 0, a win that is not strictly increasing or leaves [0, nt], a outside
 * [0, 65536], x0 not finite: XMHW_ERR_INVALID.  Then nothing is launched for ns == 0 or an empty coarse grid; then a NULL
 * ts_dev, wi_dev, out_dev or n_range_dev is XMHW_ERR_INVALID.  Asynchronous on `stream`.
 * A lane owns one coarse cell and walks its fy rows x fx columns x len steps with three sums in registers; fx = 1, 2, 4 read
 * a row's samples in one load of the lane's width where the pointers, ld and nx keep every lane aligned
 * (csrc/kernels_coarsen.hip, csrc/coarsen_index.h).  xmhw_set_coarsen_variant (process-wide; tests and measurements): 0 = the
 * widest loads the call allows (the default), 1 = loads of one sample, 2 = the run-time column loop of any other fx.
 * xmhw_set_coarsen_chunk (likewise): the windows a workgroup takes per chunk, 0 = automatic.  Same results for every value. */
#define XMHW_COARSEN_MAX_VOLUME      4096
#define XMHW_COARSEN_MAX_WEIGHT_BITS 24
int xmhw_set_coarsen_variant(int32_t variant);        /* tests and measurements; 0 = automatic */
int xmhw_set_coarsen_chunk(int32_t windows);          /* tests and measurements; 0 = automatic */
/* which instantiation a call with these arguments takes under the variant in force (no HIP call): 0 = the column loop,
 * 1 = fx 1, 2 / 3 = fx 2 with loads of one / two samples, 4 / 5 = fx 4 with loads of one / four samples                  */
int xmhw_coarsen_class(const void *ts_dev, const int32_t *wi_dev, int64_t ld, int32_t nx, int32_t itemsize, int32_t fx);
int xmhw_coarsen_f32(const float *ts_dev, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy,
                     int32_t ncx, const int32_t *wi_dev, double x0, int32_t a, const int32_t *win_host, int32_t ns,
                     float *out_dev, int64_t ldo, int64_t *wsum_dev, int32_t *n_dev, int64_t *n_range_dev, void *stream);
int xmhw_coarsen_f64(const double *ts_dev, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy,
                     int32_t ncx, const int32_t *wi_dev, double x0, int32_t a, const int32_t *win_host, int32_t ns,
                     double *out_dev, int64_t ldo, int64_t *wsum_dev, int32_t *n_dev, int64_t *n_range_dev, void *stream);

/* ---- regrid(): first-order conservative remapping between two rectilinear grids ---- *
 * The front-end stage that brings two products onto one grid: OISST (ascending latitude, centres at x.125) onto ERA5
 * (descending, centres at x.00), either onto a model's 1 degree grid.  coarsen() nests integer blocks of one grid; this
 * stage takes any two lat-lon grids.  Rectilinear grids make the overlap of the destination cell (J, I) with the source cell
 * (j, i) a product, the overlap of row J with row j times the overlap of column I with column i: the device sees two small
 * CSR tables and no 2-D weight matrix.
 *
 * Source series.  ts_dev[nt][ld] is x[t][j][i], UNCOMPACTED on the ny x nx grid, longitude the fast axis, float32 or
 * float64, ld >= ny * nx, NaN = no sample.
 *
 * Row table (host arrays).  row_first[my], row_ptr[my + 1] (row_ptr[0] = 0, non-decreasing): destination row J reads the
 * source rows row_first[J] + r, r < row_ptr[J + 1] - row_ptr[J] -- consecutive indices in memory order, so ascending or
 * descending latitude makes no difference to the device -- under the int32 weights ay[row_ptr[J] + r]; wy[J] is the row's
 * full extent in the same unit.  Column table.  col_first[mx], col_ptr[mx + 1], ax[], wx[mx] likewise; with periodic != 0
 * the source column is (col_first[I] + k) mod nx, and a run may cross the seam.
 *
 * Caps.  0 <= ay, ax <= XMHW_REGRID_MAX_WEIGHT = 2^12; a run holds at most XMHW_REGRID_MAX_RUN = 64 entries per axis, so at
 * most 4,096 samples feed a cell and w = ay * ax <= 2^24, the bound of coarsen(); the weights of a run sum to its extent at
 * most and wy, wx <= XMHW_REGRID_MAX_EXTENT = 2^18; row_first + count <= ny; col_first + count <= nx, or, periodic,
 * 0 <= col_first < nx and count <= nx.  A run of 0 entries is allowed: that cell is NaN with n = 0.
 *
 * Sums.  For (t, J, I), over the pairs (r, k) with w = ay * ax > 0 whose sample is not NaN:
 *   xq = rint(((double)x - x0) * 2^XMHW_REGION_SERIES_BITS)     (the fixed point of region_series(), in float64 as written)
 *   a pair with |x - x0| >= 2^7, or an infinite x, is left out of all sums and counted in *n_range_dev (int64, ADDED to):
 *   the count is of (destination, source) PAIRS, because a source sample may feed several cells or none
 *   n += 1, wsum += w, xsum += w * xq                            (exact integers)
 * |xsum| <= 2^12 * 2^24 * 2^23 = 2^59, wsum * 65536 <= 2^52 and a * wy * wx <= 2^52.  The sums are exactly separable,
 * sum_r ay * (sum_k ax * ...), and the kernel uses that.
 *
 * Validity.  n >= 1 and wsum * 65536 >= a * wy[J] * wx[I]; a is an integer in [0, 65536], the least covered share in
 * 65536ths; equality counts as valid.
 *
 * Output.  out_dev[t][J * mx + I] = x0 + ((double)xsum / (double)wsum) / 65536.0, in float64 exactly as written, rounded
 * once to the sample type; NaN for an invalid cell.  out_dev[nt][ldo] (ldo >= my * mx) is WRITTEN, not added to; columns
 * past my * mx are never touched.  wsum_dev (int64 [nt][ldo]) and n_dev (int32 [nt][ldo]) are optional: NULL = not written.
 * The finish is two integer-to-double conversions, one correctly rounded division, an exact scaling and one add (the build
 * uses -ffp-contract=off): numpy reproduces every bit.  The result does not depend on launch geometry, step chunks, time
 * blocks or the path taken.
 *
 * Refusals, in this order and before the first HIP call.  (1) Over the tables that can be read (all pointers of the axis
 * there, the pointer table from 0 and non-decreasing): a run longer than 64, an extent above 2^18, a weight above 2^12; then
 * ny * nx or my * mx of 2^31 and more: XMHW_ERR_UNSUPPORTED.  (2) A negative nt, ny, nx, my or mx, ld < ny * nx,
 * ldo < my * mx; tables that cannot be read, a negative weight, weights of a run that exceed its extent, a run that leaves
 * the source grid (rows first, then columns); a outside [0, 65536]; x0 not finite: XMHW_ERR_INVALID.  (3) Nothing is
 * launched for nt == 0 or an empty destination grid.  (4) A NULL ts_dev, out_dev or n_range_dev is XMHW_ERR_INVALID.  The
 * tables are then uploaded as one cached device table (the time blocks of a call reuse it).  Asynchronous on `stream`.
 *
 * A lane owns one destination cell; a workgroup is one destination row x 256 columns.  Two paths give identical bits
 * (csrc/kernels_regrid.hip, csrc/regrid_index.h): direct -- every lane loads and converts its own samples, the samples of
 * four steps requested together, any table within the caps -- and staged -- the workgroup loads the source footprint of its
 * tile once per step, converts every sample once into an LDS dword and the lanes read their words from LDS; possible where
 * (the longest row run) x (the widest column span of a tile) fits 16,384 dwords.  The automatic choice takes the staged path
 * where it measured faster: that product is 4,096 dwords at most and the span holds two source columns per lane and more.
 * xmhw_set_regrid_variant (process-wide; tests and measurements): 0 = automatic, 1 = direct, 2 = staged where it fits.
 * xmhw_set_regrid_chunk (likewise): the steps a workgroup takes per chunk, 0 = automatic.  Same results for every value.  */
#define XMHW_REGRID_MAX_RUN    64
#define XMHW_REGRID_MAX_WEIGHT 4096
#define XMHW_REGRID_MAX_EXTENT 262144
int xmhw_set_regrid_variant(int32_t variant);         /* tests and measurements; 0 = automatic */
int xmhw_set_regrid_chunk(int32_t steps);             /* tests and measurements; 0 = automatic */
/* which path a call with these host tables takes under the variant in force (no HIP call): 1 = direct, 2 = staged;
 * 0 = the tables describe no call (a negative size, nx < 1, a NULL table, a run that is negative, longer than 64 or
 * leaves the grid)                                                                                                       */
int xmhw_regrid_class(int32_t nx, int32_t my, int32_t mx, const int32_t *row_ptr_host, const int32_t *col_first_host,
                      const int32_t *col_ptr_host, int32_t periodic);
int xmhw_regrid_f32(const float *ts_dev, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx,
                    const int32_t *row_first_host, const int32_t *row_ptr_host, const int32_t *ay_host, const int32_t *wy_host,
                    const int32_t *col_first_host, const int32_t *col_ptr_host, const int32_t *ax_host, const int32_t *wx_host,
                    int32_t periodic, double x0, int32_t a, float *out_dev, int64_t ldo, int64_t *wsum_dev, int32_t *n_dev,
                    int64_t *n_range_dev, void *stream);
int xmhw_regrid_f64(const double *ts_dev, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx,
                    const int32_t *row_first_host, const int32_t *row_ptr_host, const int32_t *ay_host, const int32_t *wy_host,
                    const int32_t *col_first_host, const int32_t *col_ptr_host, const int32_t *ax_host, const int32_t *wx_host,
                    int32_t periodic, double x0, int32_t a, double *out_dev, int64_t ldo, int64_t *wsum_dev, int32_t *n_dev,
                    int64_t *n_range_dev, void *stream);

/* ---- the sharded path: cells split across the GPUs of a node, ONE gather at the end ------- *
 * Replaces the reference's collect, dask.compute(climls) + xr.concat(dim='cell')
 * (xmhw/xmhw.py:197, :210-211).  Cells are independent (xmhw/xmhw.py:184-196), so rank r runs the
 * hot path above on its own contiguous block of columns [c0_r, c0_r + cols_r) -- the caller simply
 * passes that block's device pointer and width to xmhw_clim_raw_* / xmhw_clim_finish -- and the
 * (rows, cols_r) float64 result blocks are gathered device-to-device over RCCL / xGMI.
 * One process per GPU; RCCL is loaded (dlopen) at the first call of this section.             */
typedef struct xmhw_comm xmhw_comm;
#define XMHW_UNIQUE_ID_BYTES 128
/* rank 0 creates the 128-byte id and hands it to the other ranks by any out-of-band means
 * (xmhw_amd/bootstrap.py uses a TCP socket; MPI_Bcast or a shared file work as well)          */
int xmhw_comm_unique_id(void *id_out);
/* collective over all ranks, on each rank's CURRENT device (xmhw_set_device first)             */
int xmhw_comm_create(int rank, int nranks, const void *id, xmhw_comm **comm);
int xmhw_comm_destroy(xmhw_comm *comm);
int xmhw_comm_info(const xmhw_comm *comm, int *rank, int *nranks);
/* metadata: every rank contributes one int64 (cell counts, table sizes, error flags) and gets
 * all of them back on the host; synchronises `stream`                                           */
int xmhw_comm_allgather_i64(xmhw_comm *comm, int64_t value, int64_t *out_host, void *stream);
/* the same in two halves: begin() queues copy-in, collective and copy-out (pinned on both ends) and
 * returns; end() waits for that work only.  One all-gather in flight per communicator.        */
int xmhw_comm_allgather_i64_begin(xmhw_comm *comm, int64_t value, void *stream);
int xmhw_comm_allgather_i64_end(xmhw_comm *comm, int64_t *out_host);
/* equal-sized byte blocks (land-mask slabs): recv_dev holds nranks * bytes_per_rank; asynchronous */
int xmhw_comm_allgather_bytes(xmhw_comm *comm, const void *send_dev, void *recv_dev,
                              size_t bytes_per_rank, void *stream);
/* THE gather: rank r sends its dense (rows, cols) float64 block; on `root`, recv_dev receives the
 * blocks one after the other in rank order, block r being (rows, cols_of_rank[r]) contiguous
 * (cols_of_rank is read on the root only and cols_of_rank[root] must equal cols; empty blocks
 * are allowed).  Grouped ncclSend / ncclRecv on `stream`, asynchronous; the caller places the
 * blocks (xmhw_memcpy2d_d2h writes block r straight into columns [c0_r, c0_r + cols_r) of a
 * row-major host array).                                                                        */
int xmhw_gather_blocks(xmhw_comm *comm, const double *send_dev, int64_t rows, int64_t cols,
                       double *recv_dev, const int64_t *cols_of_rank, int root, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XMHW_AMD_H */
