// kernels.h -- host-callable launchers (defined in the .hip files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xmhw {

struct DevChunk { int32_t warm_start, begin, end; };
// int16-packed input (CF packing: value = code * scale_factor + add_offset, _FillValue -> NaN; what xmhw_decode() would
// write out, see kernels_ingest.hip) read by the kernels directly: the sorted-list kernel, its recomputation and the
// leftover kernel take the codes and this recipe instead of a decoded copy of the series (capi.cpp: xmhw_clim_raw_i16).
//   mode 1  float32 decode: a sample is float(code) * sf + of, two float32 roundings -- the float32 series xarray (and
//           xmhw_decode) would hand over; the kernels key and sum exactly those values;
//   mode 2  float64 decode (float64 packing attributes): code -> value is monotone, so the kernels key float(code)
//           (exact) and decode only the two selected codes and the mean of the codes: double(code) * s + o;
//   mode 3  no packing attributes: a sample is float(code).
struct PackedI16 {
    int32_t mode = 0;
    int32_t fill = 0x7FFFFFFF;   // the code that means "missing" (0x7FFFFFFF: none)
    int32_t swap = 0;            // the codes are big-endian
    int32_t key_neg = 0;         // the kernel keys the NEGATED sample (cold spells; mode 2: XOR a negative scale_factor)
    int32_t val_neg = 0;         // mode 2: the outputs are those of the negated series (cold spells)
    float sf = 1.0f, of = 0.0f;
    double s = 1.0, o = 0.0;
};
// a chunk of the sorted-list kernel: its table / flag rows start at trow0 (row of step warm_start)
// direct_lo / direct_hi: 0, or -- a chunk the kernel settles directly (plan.h: SortedPlan::direct) -- its pooled tracks as
// a bit set (track k = bit k)
struct DevSortedChunk { int32_t warm_start, begin, end, trow0; uint32_t direct_lo, direct_hi; };

// generic kernel (any plan): thread per (cell, row)
template <typename T>
hipError_t launch_generic(const T* ts, int64_t Tn, int64_t C, int64_t ld, const int32_t* row_ptr,
                          const int32_t* centres, int32_t D, int32_t w, double q, int negate,
                          double* thresh, double* seas, int64_t ldo, hipStream_t stream,
                          const uint32_t* run_flag = nullptr);   // non-NULL: return at once unless *run_flag != 0

// ring kernel (fast path).  Returns hipErrorInvalidValue if (w, yps) is not instantiated.
bool ring_supported(int32_t w, int32_t yps, int32_t subs, int elem_bytes);
// tracks per lane (0 if none) and lanes per cell (8, or 16 for records of 49..96 tracks) of the
// float32 ring kernel that covers ntracks tracks
int32_t ring_pick(int32_t w, int32_t ntracks, int elem_bytes, int32_t* subs_out);
hipError_t launch_ring_f32(const float* ts, int64_t C, int64_t ld, const uint32_t* table,
                           int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                           int32_t w, int32_t yps, int32_t subs, double q, int negate, double* thresh,
                           double* seas, int64_t ldo, hipStream_t stream,
                           unsigned long long* stats = nullptr);

// second-generation float32 ring kernel (kernels_ring2.hip): tracks dealt y-major; variant = its layouts 8 / 10 / 12
// (8 / 4 / 16 lanes per cell; route.cpp maps every layout number to its kernel generation and lanes)
int32_t ring2_pick_yps(int32_t w, int32_t ntracks, int32_t variant);   // tracks per lane, 0 if not instantiated
bool ring2_narrowing_supported(int32_t w, int32_t yps, int32_t variant);   // float64 -> float32 narrowing instantiation exists
hipError_t launch_narrow_probe(const double* ts, int64_t Tn, int64_t C, int64_t ld, uint32_t* narrow_flag, hipStream_t stream);
hipError_t launch_ring2_f32_narrowing(const double* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                                      const uint32_t* sflags, int32_t step_min, const DevChunk* chunks,
                                      int32_t nchunks, int32_t w, int32_t yps, int32_t ntracks, int32_t variant,
                                      double q, int negate, double* thresh, double* seas, int64_t ldo,
                                      hipStream_t stream, uint32_t* narrow_flag);
bool ring2_f32_supported(int32_t w, int32_t yps, int32_t variant);         // float32 instantiation exists
bool ring2_x64_supported(int32_t w, int32_t yps, int32_t variant);         // 64-bit (high / low key word) instantiation exists
hipError_t launch_ring2_f64(const double* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                            const uint32_t* sflags, int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                            int32_t w, int32_t yps, int32_t ntracks, int32_t variant, double q, int negate,
                            double* thresh, double* seas, int64_t ldo, hipStream_t stream, const uint32_t* run_flag);
bool ring_stats_built();                                                // the counter twins exist (-DXMHW_RING_STATS)
hipError_t launch_ring2_f32(const float* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                            const uint32_t* sflags, int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                            int32_t w, int32_t yps, int32_t ntracks, int32_t variant, double q, int negate,
                            double* thresh, double* seas, int64_t ldo, hipStream_t stream,
                            unsigned long long* stats = nullptr);

// third-generation float32 ring kernel (kernels_ring3.hip): per-cell histogram in LDS + band compaction;
// 8, 4 or 2 lanes per cell (layouts 20, 21 and 22), w = 5
int32_t ring3_pick_yps(int32_t w, int32_t ntracks, int32_t subs);
bool ring3_supported(int32_t w, int32_t yps, int32_t subs);
hipError_t launch_ring3_f32(const float* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                            const uint32_t* sflags, int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                            int32_t w, int32_t yps, int32_t subs, int32_t ntracks, double q, int negate,
                            double* thresh, double* seas, int64_t ldo, hipStream_t stream,
                            unsigned long long* stats = nullptr);

// fifth generation (kernels_sorted.hip): sorted row-lists in LDS + a parallel merge-select; 2 lanes per cell, w = 5,
// float32 (or int16 codes read in place), on its own chunks and table rows (plan.h: sorted_plan).  A cell-row the select
// cannot settle (a row-list too short for it) is recomputed exactly inside the kernel, by the whole wave, from the samples.
int32_t sorted_pick_yps(int32_t w, int32_t ntracks);     // tracks per lane, 0 if not instantiated
int32_t sorted_pick_k(int32_t w, int32_t ntracks);       // keys kept per row-list, 0 if not instantiated
int32_t sorted_lds_bytes(int32_t w, int32_t ntracks);    // LDS of a wave (32 cells): 11 lists x the ranks kept in LDS, in 1,280-byte pieces
// the device behaviour the kernel's rank-major lists rely on (an LDS read outside the allocation returns 0): *d_bad = 0 if it holds
hipError_t sorted_lds_probe(uint32_t* d_bad, hipStream_t stream);
hipError_t launch_sorted_f32(const float* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                             const uint32_t* sflags, const DevSortedChunk* chunks, int32_t nchunks,
                             int32_t w, int32_t yps, int32_t ntracks, double q, int negate, double* thresh, double* seas,
                             int64_t ldo, hipStream_t stream, unsigned long long* stats = nullptr,
                             int32_t ndirect = 0);      // ndirect: how many of the chunks are marked direct
// the sorted-list kernel on int16 codes (instantiated for the same records as launch_sorted_f32)
hipError_t launch_sorted_i16(const int16_t* codes, const PackedI16& pk, int64_t C, int64_t ld, int64_t Tn,
                             const uint32_t* table, const uint32_t* sflags, const DevSortedChunk* chunks, int32_t nchunks,
                             int32_t w, int32_t yps, int32_t ntracks, double q, int negate, double* thresh, double* seas,
                             int64_t ldo, hipStream_t stream);

// fourth-generation float32 ring kernel (kernels_ring4.hip): a windowed key store in LDS instead of histogram + band
// compaction; same lane layouts and step tables as the third generation (layouts 30 / 31 / 32 = 8 / 4 / 2 lanes)
int32_t ring4_pick_yps(int32_t w, int32_t ntracks, int32_t subs);
bool ring4_supported(int32_t w, int32_t yps, int32_t subs);
bool ring4_stats_built();
hipError_t launch_ring4_f32(const float* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                            const uint32_t* sflags, int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                            int32_t w, int32_t yps, int32_t subs, int32_t ntracks, double q, int negate,
                            double* thresh, double* seas, int64_t ldo, hipStream_t stream,
                            unsigned long long* stats = nullptr);

// genuinely float64 samples: the 64-bit mode (high / low key words) of the third-generation kernel, 8 lanes per cell
bool ring3_x64_supported(int32_t w, int32_t yps, int32_t subs);
hipError_t launch_ring3_f64(const double* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                            const uint32_t* sflags, int32_t step_min, const DevChunk* chunks, int32_t nchunks,
                            int32_t w, int32_t yps, int32_t subs, int32_t ntracks, double q, int negate, double* thresh,
                            double* seas, int64_t ldo, hipStream_t stream, const uint32_t* run_flag);
// the same for float64 input whose samples are float32-representable (see launch_ring2_f32_narrowing)
bool ring3_narrowing_supported(int32_t w, int32_t yps, int32_t subs);
hipError_t launch_ring3_f32_narrowing(const double* ts, int64_t C, int64_t ld, int64_t Tn, const uint32_t* table,
                                      const uint32_t* sflags, int32_t step_min, const DevChunk* chunks,
                                      int32_t nchunks, int32_t w, int32_t yps, int32_t subs, int32_t ntracks, double q,
                                      int negate, double* thresh, double* seas, int64_t ldo, hipStream_t stream,
                                      uint32_t* narrow_flag);

// float64 input through the float32 ring kernel: zeroes narrow_flag, probes the series, runs the
// kernel with samples narrowed on load; narrow_flag != 0 afterwards: some sample is not float32-
// representable and the outputs are garbage (queue launch_ring2_f64(..., run_flag = narrow_flag) behind)
hipError_t launch_ring_f32_narrowing(const double* ts, int64_t Tn, int64_t C, int64_t ld, const uint32_t* table,
                                     int32_t step_min, const DevChunk* chunks, int32_t nchunks, int32_t w,
                                     int32_t yps, int32_t subs, double q, int negate, double* thresh, double* seas,
                                     int64_t ldo, hipStream_t stream, unsigned long long* stats,
                                     uint32_t* narrow_flag);

// Feb-29 substitution + circular running mean, per cell over present groups
hipError_t launch_finish(const double* th_in, const double* se_in, int64_t C, int64_t ldo, int32_t D,
                         int32_t i59, int32_t i60, int32_t i61, int feb29_fix, int smooth,
                         int32_t width, double* th_out, double* se_out, hipStream_t stream,
                         uint8_t* flags = nullptr);      // C bytes of scratch: enables the one-pass kernel (width 31)

template <typename T>
hipError_t launch_land_mask(const T* ts, int64_t Tn, int64_t C, int64_t ld, int anynans,
                            uint8_t* keep, hipStream_t stream);

hipError_t launch_land_mask_i16(const int16_t* codes, int64_t Tn, int64_t C, int64_t ld, int16_t fill_raw, int anynans,
                                uint8_t* keep, hipStream_t stream);

template <typename T>
hipError_t launch_gather_cells(const T* in, int64_t rows, int64_t ld_in, const int64_t* index, int64_t n,
                               T* out, int64_t ld_out, hipStream_t stream);
hipError_t launch_scatter_cells(const double* in, int64_t rows, int64_t ld_in, const int64_t* index,
                                int64_t n, double* out, int64_t ld_out, int64_t ncols_out,
                                hipStream_t stream);

// detect() front end: exceedance + event filter + gap joining, thread per cell
template <typename T>
hipError_t launch_detect(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                         const int32_t* row_of_t, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                         int32_t negate, int32_t* events, int32_t* start, int32_t* end, uint8_t* bthresh,
                         int64_t ldo, int32_t* nevents, hipStream_t stream);

hipError_t launch_count_events(const int32_t* start, int64_t Tn, int64_t C, int64_t ldo, int32_t* nevents,
                               hipStream_t stream);

// per-event statistics into a compact table (kEventColumns doubles per event)
constexpr int kEventColumns = 31;
template <typename T>
hipError_t launch_event_stats(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas,
                              const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                              const int32_t* events, int64_t ldo, const int64_t* offsets, double* table,
                              hipStream_t stream);

// table-only define_events() (kernels_events.hip): exceedance bits, run walk, per-event statistics
hipError_t launch_floor_to_f32(const double* th, int64_t rows, int64_t cols, int64_t ldi, float* out, int64_t ldo,
                               hipStream_t stream);
template <typename T, typename TH>
hipError_t launch_exceed_bits(const T* ts, int64_t Tn, int64_t C, int64_t ld, const TH* thresh, int64_t ldt,
                              const int32_t* row_of_t, int32_t negate, uint64_t* bits, int64_t ldb,
                              hipStream_t stream);
template <typename T, typename TH, int TILE>
hipError_t launch_exceed_bits_tiled(const T* ts, int64_t C, int64_t ld, const TH* thresh, int64_t ldt, int64_t D,
                                    const int32_t* tile_begin, int32_t ntiles, const int32_t* chunk_t0,
                                    const int32_t* chunk_i0, const int32_t* chunk_n, int32_t negate, uint64_t* bits,
                                    int64_t ldb, hipStream_t stream);
hipError_t launch_events_from_bits(const uint64_t* bits, int64_t Tn, int64_t C, int64_t ldb, int32_t min_duration,
                                   int32_t join_gaps, int32_t max_gap, const int64_t* offsets, int32_t* nevents,
                                   double* table, hipStream_t stream);
template <typename T>
hipError_t launch_event_stats_sparse(const T* ts, int64_t Tn, int64_t ld, const double* seas, const double* thresh,
                                     int64_t ldc, const int32_t* row_of_t, int32_t negate, int64_t n_events,
                                     double* table, hipStream_t stream);

// exclusive prefix sum of per-cell event counts into int64 table offsets [n+1]; block_sums: scratch of
// (n + 1023) / 1024 + 1 int64
hipError_t launch_offsets_from_counts(const int32_t* counts, int64_t n, int64_t* offsets, int64_t* block_sums,
                                      hipStream_t stream);

// per-step columns of mhw_df(): out [8][T][ldv] f64, dur [4][T][ldv] u8
template <typename T>
hipError_t launch_event_intermediate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas,
                                     const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                     const int32_t* events, int64_t ldo, double* out, int64_t ldv, uint8_t* dur,
                                     hipStream_t stream);

// block_average() (kernels_stats.hip): segmented reductions keyed by (cell, year bin); out[stat][bin][cell]
constexpr int kBlockEventStats = 15;
hipError_t launch_block_events(const double* table, const int64_t* offsets, int64_t C, const int32_t* bin_of_t, int64_t Tn,
                               int32_t nbins, int32_t mtime_col, double* out, int64_t ldo, hipStream_t stream);
template <typename T>
hipError_t launch_block_time(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* cats, int64_t ldcat,
                             const int32_t* bin_of_t, int32_t nbins, double* out, int64_t ldo, hipStream_t stream);

// mhw_rank() (kernels_rank.hip): per-cell ranks (largest = 1, ties: the later event first, NaN -> NaN) and
// return periods (n_years + 1) / rank of the table columns col[0..ncols), written to column out[k] of the
// rows of rank / rp (leading dimension ld_out).  One launch covers a window of table columns
// [cmin, cmin + span), span <= kRankWindow, ncols <= kRankWindow.  Scratch: item_counts[C] int32,
// item_off[C + 1] int64, scan_scratch (C + 1023) / 1024 + 1 int64, next_item one uint64.
constexpr int kRankWindow = 16;
struct RankColumns {
    int32_t col[kRankWindow];
    int32_t out[kRankWindow];
    int32_t ncols, cmin, span;
};
hipError_t launch_event_rank(const double* table, int64_t ld_table, const int64_t* offsets, int64_t C,
                             const RankColumns& rc, double n_years, double* rank, double* rp, int64_t ld_out,
                             int32_t* item_counts, int64_t* item_off, int64_t* scan_scratch,
                             unsigned long long* next_item, hipStream_t stream);

// mean_trend() (kernels_trend.hip): per (cell, statistic) trends of the block_average() planes y[stat][nb][ld]
// along the abscissa x[nb] (device, strictly increasing), NaN blocks left out.  OLS writes out[what][stat][ldo] with
// what = mean, trend, dtrend (tcrit[dof], device, nb - 1 entries, entry 0 unused); Theil-Sen writes what = trend,
// mean, mk_s, mk_var and takes at most kTrendMaxBlocks blocks (its slopes live in LDS).
constexpr int kTrendMaxBlocks = 128;
hipError_t launch_trend_ols(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                            const double* tcrit, double* out, int64_t ldo, hipStream_t stream);
hipError_t launch_trend_theil_sen(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                                  double* out, int64_t ldo, hipStream_t stream);

// detrend() (kernels_fit.hip): launch_series_fit solves, per cell of the series ts[T][ld], the least squares of its
// samples on the design matrix basis[T][P] (device, float64, shared by all cells) over the steps with weight[t] != 0
// (device, NULL: all) and a non-NaN sample, and writes coef[P][ldc] (NaN for a failed cell: fewer than `need`
// contributing samples, a contributing +-Inf, a Cholesky pivot not above 1e-6 of its diagonal entry) and nvalid[C]
// (may be NULL).  gram: kFitGramWords doubles, flags: C bytes of device workspace, written by the call.  launch_series_remove
// subtracts sum_{k<R} coef[k] basis[t][k] from every sample in place.  P <= kFitMaxTerms.
constexpr int kFitMaxTerms = 10;
constexpr int kFitGramWords = 64;
template <typename T>
hipError_t launch_series_fit(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P,
                             const uint8_t* weight, int32_t need, double* gram, uint8_t* flags, double* coef, int64_t ldc,
                             int32_t* nvalid, hipStream_t stream);
template <typename T>
hipError_t launch_series_remove(T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P, int32_t R,
                                const double* coef, int64_t ldc, hipStream_t stream);

// mhw_coverage() (kernels_coverage.hip): event_day_bits turns the exceedance words of exceed_bits into the per-day
// in-event bitmap inev[w][ldi] (steps first..last of every filtered, gap-joined event; zeroed here first).  The stage
// entries that take such a bitmap get it through entry_common.h's event_day_bitmap; what a stage adds from it, its
// limits and its launches stand in the stage's own kernel file, beside its C entries.
hipError_t launch_event_day_bits(const uint64_t* bits, int64_t Tn, int64_t C, int64_t ldb, int32_t min_duration,
                                 int32_t join_gaps, int32_t max_gap, uint64_t* inev, int64_t ldi, hipStream_t stream);

// mhw_objects() (kernels_objects.hip): launch_event_objects groups the table rows (runs of days start..end in one cell,
// rows of cell c = offsets[c]..offsets[c + 1], in time order) into connected components: rows of DIFFERENT cells are
// linked iff one cell is among the other's K neighbours nbr[c][K] (-1: none) and start_a <= end_b + gap and start_b <=
// end_a + gap.  Writes cell_of_row[n] and root[n] = the smallest row of the row's component.  launch_object_reduce
// reduces the rows into the per-object slots slot[r] in [0, n_slots) (root itself is a valid slot array); it initialises
// its outputs.  intensity_max doubles as the 64-bit key accumulator until the last kernel.
hipError_t launch_event_objects(const int32_t* start, const int32_t* end, int64_t n, const int64_t* offsets, int64_t C,
                                const int32_t* nbr, int32_t K, int32_t gap, int32_t* cell_of_row, int32_t* root,
                                hipStream_t stream);
hipError_t launch_object_reduce(const int32_t* start, const int32_t* end, const double* imax, int64_t n,
                                const int32_t* cell_of_row, const int64_t* offsets, const int64_t* wq,
                                const int32_t* slot, int64_t n_slots, int32_t* n_events, int32_t* n_cells,
                                int32_t* time_start, int32_t* time_end, int64_t* cell_days, int64_t* area_days_q,
                                double* intensity_max, int32_t* peak_row, hipStream_t stream);

// mhw_tracks() (kernels_tracks.hip): the daily series of the selected objects as one ragged array of L entries plus a
// sentinel.  slot[r] in [0, n_slots) is the position of row r's object in the selection (anything else: the row does
// nothing); object i owns the entries offsets[i]..offsets[i + 1] - 1, one per day from time_start[i]; offsets[n_slots]
// == L.  vec[4][ldv] holds the four per-cell addends (area weight and three moment terms).  Initialises and fills
// n_cells[L + 1] and sums[4][ld] (ld >= L + 1): a scatter into difference arrays, then an inclusive scan in place by
// reduce-then-scan over tiles of kTracksTile entries (scratch: object_tracks_scratch_bytes(L + 1)).  Entry L of every
// channel ends as 0.  *n_bad counts the rows left out because their days or cell do not fit (0 for consistent inputs).
constexpr int kTracksTile = 1024;
constexpr int kTracksChannels = 5;
size_t object_tracks_scratch_bytes(int64_t L1);
hipError_t launch_object_tracks(const int32_t* start, const int32_t* end, int64_t n, const int32_t* slot,
                                const int32_t* cell_of_row, int64_t C, const int64_t* vec, int64_t ldv,
                                const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L,
                                int32_t* n_cells, int64_t* sums, int64_t ld, int32_t* n_bad, int64_t* scratch,
                                hipStream_t stream);

// mhw_track_parts() (kernels_parts.hip): the connected parts of every selected object on each of its days, in the
// ragged layout of launch_object_tracks (entry offsets[slot] + (t - time_start[slot])).  The rows of cell c are
// row_offsets[c]..row_offsets[c + 1] in time order; nbr[C][K] lists the spatial neighbours (-1: none); only rows of
// equal slot are united.  vox_off[n + 1] is the exclusive prefix sum of the durations of the selected rows (0 for the
// others), V = vox_off[n] the number of voxels.  Initialises and fills n_parts[L], cells_largest[L] (int32) and
// area_largest_q[L] (the largest sum of wq over one part; an independent maximum).  scratch: kPartsVoxelBytes per voxel
// (area int64[V], parent int32[V], cells int32[V]), object_parts_scratch_bytes(V).  *n_bad counts the selected rows
// left out because their days, cell or voxel numbers do not fit (0 for consistent inputs).
constexpr int kPartsVoxelBytes = 16;
size_t object_parts_scratch_bytes(int64_t V);
hipError_t launch_object_parts(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row,
                               int64_t n, const int64_t* row_offsets, int64_t C, const int32_t* nbr, int32_t K,
                               const int64_t* wq, const int64_t* vox_off, int64_t V, const int32_t* time_start,
                               const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* n_parts, int32_t* cells_largest,
                               int64_t* area_largest_q, int32_t* n_bad, void* scratch, hipStream_t stream);

// mhw_track_genealogy() (kernels_genealogy.hip): the links between the parts of consecutive days of every selected
// object, in the ragged layout and on the rows and voxels of launch_object_parts.  Initialises and fills counts[6][L]
// (int32, one array of L per field, in the order of the kGenealogy* indices below), writes the *n_edges distinct
// links as (root voxel of the earlier part << 32) | root voxel of the later part to edges[edge_capacity] in arbitrary
// order (a root is the smallest voxel number of its part) and sets *n_bad (rows left out, as launch_object_parts) and
// *overflow (nonzero: the hash set was full, edge_capacity did not bound the number of keys).  edge_capacity >= the
// number of (row, day) pairs with a next day in the row plus the row pairs of one cell and slot that touch in time.
// scratch: the hash set of object_genealogy_table_slots(edge_capacity) slots of kGenealogySlotBytes, then
// kGenealogyVoxelBytes per voxel (parent, indeg, outdeg int32[V]); object_genealogy_scratch_bytes(V, edge_capacity).
constexpr int kGenealogyVoxelBytes = 12;
constexpr int kGenealogySlotBytes = 8;
constexpr int kGenealogyFields = 6;
constexpr int kGenealogyParts = 0, kGenealogyLinks = 1, kGenealogyBorn = 2, kGenealogyMerged = 3, kGenealogyEnded = 4,
              kGenealogySplit = 5;
int64_t object_genealogy_table_slots(int64_t edge_capacity);
size_t object_genealogy_scratch_bytes(int64_t V, int64_t edge_capacity);
hipError_t launch_object_genealogy(const int32_t* start, const int32_t* end, const int32_t* slot,
                                   const int32_t* cell_of_row, int64_t n, const int64_t* row_offsets, int64_t C,
                                   const int32_t* nbr, int32_t K, const int64_t* vox_off, int64_t V,
                                   const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L,
                                   int32_t* counts, uint64_t* edges, int64_t edge_capacity, int64_t* n_edges,
                                   int32_t* n_bad, int32_t* overflow, void* scratch, hipStream_t stream);

// mhw_track_shape() (kernels_shape.hip): the outline of every selected object on each of its days, in the ragged layout
// and on the rows of launch_object_parts (no voxels, no scratch).  faces[C][4] names what lies across the four faces of
// every cell (dim 0 minus, dim 0 plus, dim 1 minus, dim 1 plus): a compact cell, or one of the kShapeFace* codes;
// lq[C][4] int64 >= 0 are their lengths.  A face to a cell that holds a fit row of the same slot on the same day is
// shared and counts nothing; any other is open.  Zeroes and fills edges[3][L] (int32) and perimeter_q[3][L] (int64),
// one array of L per class in the order of the kShape* indices, and cells_edge[L] (int32, the footprint cells with at
// least one counted face).  *n_bad counts the selected rows left out because their days or cell do not fit, and the
// rows with a face value outside [kShapeFaceFolded, C) (0 for consistent inputs).
constexpr int kShapeClasses = 3;
constexpr int kShapeOpen = 0, kShapeCoast = 1, kShapeBorder = 2;
constexpr int kShapeFaceCoast = -1, kShapeFaceBorder = -2, kShapeFaceFolded = -3;
hipError_t launch_object_shape(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row,
                               int64_t n, const int64_t* row_offsets, int64_t C, const int32_t* faces, const int64_t* lq,
                               const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* edges,
                               int64_t* perimeter_q, int32_t* cells_edge, int32_t* n_bad, hipStream_t stream);

// mhw_track_intensity() (kernels_track_intensity.hip): the per-voxel pass over one slab of n compacted cells.  The slab's
// table rows (start / end / slot, n_rows of them, the rows of cell c = row_offsets[c]..row_offsets[c + 1], in time
// order) are walked together with the steps of a chunk of kTrackIntensityChunk steps; a voxel of a row whose slot is in
// [0, n_slots) ADDS to entry offsets[slot] + (t - time_start[slot]) of n_valid / wsum_i / isum_q / cat_cells[4][ldcat]
// and raises the 64-bit key kept in intensity_max (launch_track_intensity_init zeroes them; launch_track_intensity_finish
// turns the keys into float64, NaN for none).  *n_range counts the voxels left out for |a| >= 2^7, *n_bad those of rows
// that do not lie within their object's entries.  row_of_t is a DEVICE array here.  combine_runs: runs of equal target
// entries among the lanes of a wave are summed by a segmented scan before the atomics.
constexpr int kTrackIntensityChunk = 64;
constexpr int kTrackIntensityBits = 16;

// The frame of a class reduction: the kernels below that reduce over TIME and keep the cell (class_days_accumulate,
// class_sums_accumulate, heat_stress_accumulate, index_regress_accumulate, lag_corr_accumulate, distribution_accumulate,
// composite_accumulate -- which keeps no addends
// and adds every (anchor, offset) pair directly; displacement_accumulate and spatial_corr_accumulate with a grid point and
// cooccur_accumulate with 64-step words in the place of the cell and the step).  Lane = cell, consecutive lanes on consecutive cells; a workgroup
// is 256 cells x a block of steps (stage_blocks.h has the block lengths); class_of_t[t] and row_of_t[t] are uniform over
// the wave.  A lane keeps the addends of the CURRENT class in registers while the class stays the same and flushes them
// when it changes and at the end of the block.  Flushes are integer atomics without a return value, issued for non-zero
// addends only, coalesced (cells are the fastest axis of every output).  Everything is an integer sum or a maximum: the
// result does not depend on the block length, the slabs, the launch geometry or the schedule.  No kernel waits for another
// workgroup.  stage_reduce.h holds the pieces: the in-event bitmap cursor, the category of a step, the fixed point of the
// sums, the run of a class, the range of a block (DESIGN.md 3.7 says which kernel takes which, and why).
//
// mhw_days_by() (kernels_class.hip): the reduction over TIME that keeps the cell.  For every class k < K of time steps
// (class_of_t[t] in [-1, K), -1 = the step counts nowhere) and cell c, over the in-event steps of the bitmap inev
// (launch_event_day_bits) with class_of_t[t] == k, class_days_accumulate ADDS to days[k][0..3][c] the steps of category
// 1, 2, 3, >= 4, to days[k][4][c] all of them, to days[k][5][c] those with a valid anomaly a = x - seas (not NaN,
// |a| < 2^7), to isum_q[k][c] the sum of rint(a * 2^kClassDaysBits) over the valid ones, and raises the 64-bit key of
// their largest a kept in intensity_max[k][c] (launch_class_days_init zeroes them; launch_class_days_finish turns the keys
// into float64, NaN for none).  Cells are the fastest axis, leading dimension ldo >= C.  *n_range counts the in-event
// steps with a not NaN and |a| >= 2^7.  row_of_t and class_of_t are DEVICE arrays here.  block_steps: the steps a workgroup
// takes per block, 0 = automatic; same results for every value.
constexpr int kClassDaysMaxClasses = 1024;
constexpr int kClassDaysChannels = 6;
constexpr int kClassDaysBits = 16;
// the finish of every float maximum kept as an order-preserving key (kernels_class.hip): keys -> float64, 0 -> NaN, in
// place, over rows x cols with leading dimension ld (rows <= 65535)
hipError_t launch_keys_to_f64(double* key, int64_t rows, int64_t cols, int64_t ld, hipStream_t stream);

// mhw_cooccurrence() (kernels_cooccur.hip): the joint event days of two detections per cell, class of time steps and lag.
// launch_event_table_bits rasterises an event table into the one-bit-per-sample, word-major, cells-minor bitmap of
// launch_exceed_bits: column j takes the rows offsets[cell[j]] .. offsets[cell[j] + 1] (in time order, 0 <= start <= end
// < Tn), every word of columns 0..C-1 is written, the bits at t >= Tn are 0.  launch_cooccur_accumulate ADDS to
// counts[k][i][0..3][c] (both, a_only, b_only, onsets; leading dimension ldo >= C) the valid pairs (t, lags[i]) of class k:
// the classes arrive as the per-word segment list seg_off[W + 1], seg_class[], seg_mask[] (a segment = a run of one
// non-negative class inside one 64-step word), lags[L] and the segments are DEVICE arrays here.  block_words: the words a
// workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kCooccurMaxClasses = 1024;
constexpr int kCooccurMaxLags = 64;
constexpr int kCooccurChannels = 4;
constexpr int kCooccurLagGroup = 8;

// heat_stress() (kernels_stress.hip): accumulated thermal stress and the class sums of the plain series.
// launch_class_sums_accumulate ADDS, per class k of the step and cell c, the steps with d = sample - x0 not NaN and
// |d| < 2^7 to n_valid[k][c] and rint(d * 2^kHeatStressBits) to sum_q[k][c]; other non-NaN d are counted in *n_range.
// launch_heat_stress_accumulate forms q(t) = rint(h * 2^kHeatStressBits) on the hot steps (h = sample - base[row_of_t[t]],
// both negated under `negate`, h0 <= h < 2^7) and S(t) = the sum of q over the W steps that end at t, and ADDS per class
// and cell: counts[k][0][c] steps with h not NaN, [1] hot steps, [2 + l] steps with S >= level_q[l]; hsum_q[k][c] the sum
// of q; raises peak_key[k][c] to S << 32 | ~t; stores S(at[j]) to snap_q[j][c]; counts the steps with h >= 2^7 or infinite
// in *n_range.  launch_heat_stress_finish splits the keys into peak_q and peak_t (0 and -1 for a class without steps).
// Cells are the fastest axis, leading dimension ldo >= C.  row_of_t, class_of_t and at are DEVICE arrays, level_q a HOST
// array here.  block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kHeatStressMaxClasses = 1024;
constexpr int kHeatStressChannels = 8;
constexpr int kHeatStressMaxLevels = 6;
constexpr int kHeatStressMaxSnapshots = 64;
constexpr int kHeatStressMaxWindow = 255;
constexpr int kHeatStressBits = 16;

// file bytes -> samples (kernels_ingest.hip): raw_type = item size of the stored type (2 int16, 4 float32,
// 8 float64), swap = the file is big-endian, optional scale/offset (CF packing) and fill value -> NaN
hipError_t launch_encode_i16(const float* in, int64_t rows, int64_t cols, int64_t ld_in, int16_t* out, int64_t ld_out,
                             double scale, double offset, int32_t fill, hipStream_t stream);
hipError_t launch_decode(const void* in, int raw_type, int swap, int64_t rows, int64_t cols, int64_t ld_in, void* out,
                         int out_itemsize, int64_t ld_out, double scale, double offset, int has_scale, int has_fill,
                         double fill, hipStream_t stream);

// ts.interpolate_na(dim=tdim, max_gap=...) on the device copy of the series, in place (kernels_ingest.hip)
hipError_t launch_pad_gaps(void* ts, int itemsize, int64_t Tn, int64_t C, int64_t ld, const double* x, double max_gap,
                           hipStream_t stream);

template <typename T>
hipError_t launch_synth(T* ts, int64_t Tn, int64_t C, int64_t ld, int64_t cell0, uint64_t seed,
                        double nan_frac, hipStream_t stream);

template <typename T>
hipError_t launch_synth_ex(T* ts, int64_t Tn, int64_t C, int64_t ld, int64_t cell0, uint64_t seed, double nan_frac,
                           double quant, double ice_frac, double rho, int64_t ice_patch, hipStream_t stream);

}  // namespace xmhw
