// regrid_index.h -- the index arithmetic of regrid() (kernels_regrid.hip): a lane owns one destination cell
// and reads the footprint that two CSR tables give it, a run of source rows (the same for the whole workgroup) by a run of
// source columns (its own).  Plain integer code without a device type, as coarsen_index.h and halo_tile.h: the kernel, the
// launcher, the C entry and a host program (tests/c/regrid_index.cpp, against brute-force tables) compile the same
// functions.  Every function checks what it is given and answers with no tile, an empty span, -1 or an empty chunk for
// anything outside.
//
//   the tile      workgroup w of my * tiles_x: destination row J = w / tiles_x, destination columns I0 .. I0 + 255 with
//                 I0 = (w % tiles_x) * 256; a wave is 64 consecutive columns of that one row
//   the span      of a tile: the contiguous source columns c0 .. c0 + width - 1 that the runs of its lanes cover, taken
//                 mod nx when the grid is periodic (a span may cross the seam).  Not periodic: c0 is the least col_first of
//                 the tile's non-empty runs.  Periodic: c0 is the col_first of the tile's first non-empty run and every run
//                 starts (col_first - c0) mod nx columns after it.  An empty tile has the span (0, 0).
//   the LDS tile  rows x width dwords, slot (r, s) = r * width + s: source row row_first[J] + r, source column
//                 regrid_source_col(c0, s): a lane reads slot (r, off + k) for entry k of its run, off its regrid_lane_offset
//   the choice    automatic: staged where the call fits, its tile is small and its lanes read two columns and more each
//                 (regrid_auto_staged: what was measured); forced for tests and measurements
//   the fit       the staged path holds one step of the largest tile: max rows x max width dwords within kRegridLdsDwords
//                 (a periodic span may be wider than nx, by a run at most: its slots past the seam hold the first columns again)
//   the chunk     workgroups along grid.y take chunks of consecutive steps
#pragma once
#include <stdint.h>

#include "stage_blocks.h"

#if defined(__HIPCC__)
#define XMHW_REGRID_FN __host__ __device__ static inline
#else
#define XMHW_REGRID_FN static inline
#endif

namespace xmhw {

constexpr int kRegridTile = 256;                     // destination columns of a workgroup
constexpr int kRegridMaxRun = 64;                    // entries of a run, per axis
constexpr int kRegridMaxWeight = 1 << 12;            // ay, ax at most
constexpr int kRegridMaxExtent = 1 << 18;            // wy, wx at most
constexpr int kRegridLdsDwords = 16384;              // the LDS tile of the staged path: 64 KiB at most
constexpr int kRegridAutoDwords = 4096;              // ... and what the automatic choice stages: 16 KiB at most

enum RegridClass : int32_t {
    kRegridNone = 0,                                 // the arguments describe no call
    kRegridDirect = 1,                               // every lane loads its samples from global memory
    kRegridStaged = 2                                // the workgroup stages its footprint in LDS, converted once
};

struct RegridSpan {
    int32_t c0, width;
};

// where the ten tables of a call lie in the one int32 table that goes to the device (items from its start)
struct RegridLayout {
    int64_t row_first, row_ptr, ay, wy, col_first, col_ptr, ax, wx, tile_c0, tile_w, total;
};
XMHW_REGRID_FN int64_t regrid_tiles_x(int32_t mx) { return mx > 0 ? (static_cast<int64_t>(mx) + kRegridTile - 1) / kRegridTile : 0; }
XMHW_REGRID_FN RegridLayout regrid_layout(int32_t my, int32_t mx, int64_t n_ay, int64_t n_ax) {
    RegridLayout l = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (my < 0 || mx < 0 || n_ay < 0 || n_ax < 0) return l;
    l.row_first = 0;
    l.row_ptr = l.row_first + my;
    l.ay = l.row_ptr + my + 1;
    l.wy = l.ay + n_ay;
    l.col_first = l.wy + my;
    l.col_ptr = l.col_first + mx;
    l.ax = l.col_ptr + mx + 1;
    l.wx = l.ax + n_ax;
    l.tile_c0 = l.wx + mx;
    l.tile_w = l.tile_c0 + regrid_tiles_x(mx);
    l.total = l.tile_w + regrid_tiles_x(mx);
    return l;
}

// workgroup w -> its destination row and first destination column; false if w is no tile of the destination grid
XMHW_REGRID_FN bool regrid_tile(int64_t w, int32_t my, int32_t mx, int32_t* J, int32_t* I0) {
    const int64_t tx = regrid_tiles_x(mx);
    if (w < 0 || my <= 0 || tx <= 0 || w >= tx * my) return false;
    *J = static_cast<int32_t>(w / tx);
    *I0 = static_cast<int32_t>(w % tx) * kRegridTile;
    return true;
}

// the longest run of a CSR pointer table ptr[m + 1] (0 for an empty or missing table)
XMHW_REGRID_FN int32_t regrid_max_run(const int32_t* ptr, int32_t m) {
    int64_t most = 0;
    if (!ptr) return 0;
    for (int32_t k = 0; k < m; ++k) {
        const int64_t c = static_cast<int64_t>(ptr[k + 1]) - ptr[k];
        most = c > most ? c : most;
    }
    return static_cast<int32_t>(most > INT32_MAX ? INT32_MAX : most);
}

// how many columns after c0 a run starts that begins at source column `first`; -1 for arguments outside the grid
XMHW_REGRID_FN int32_t regrid_lane_offset(int32_t first, int32_t c0, int32_t nx, bool periodic) {
    if (nx < 1 || first < 0 || first >= nx || c0 < 0 || c0 >= nx) return -1;
    const int32_t d = first - c0;
    if (d >= 0) return d;
    return periodic ? d + nx : -1;
}

// the source column behind slot s of a span that starts at c0: taken mod nx across a periodic seam, -1 outside the grid
XMHW_REGRID_FN int32_t regrid_source_col(int32_t c0, int32_t s, int32_t nx, bool periodic) {
    if (nx < 1 || c0 < 0 || c0 >= nx || s < 0) return -1;
    const int64_t c = static_cast<int64_t>(c0) + s;
    if (c < nx) return static_cast<int32_t>(c);
    return periodic ? static_cast<int32_t>(c % nx) : -1;
}

// the span of the tile whose first destination column is I0 (the lanes I0 .. min(I0 + 256, mx) - 1).  The tables must be
// valid for the call (the C entry checks them); anything else gives the empty span.
XMHW_REGRID_FN RegridSpan regrid_tile_span(const int32_t* col_first, const int32_t* col_ptr, int32_t mx, int32_t nx,
                                           bool periodic, int32_t I0) {
    RegridSpan sp = {0, 0};
    if (!col_first || !col_ptr || mx < 1 || nx < 1 || I0 < 0 || I0 >= mx) return sp;
    const int32_t I1 = mx - I0 < kRegridTile ? mx : I0 + kRegridTile;
    int64_t c0 = -1, end = 0;
    if (periodic) {
        for (int32_t I = I0; I < I1; ++I) {
            const int64_t cnt = static_cast<int64_t>(col_ptr[I + 1]) - col_ptr[I];
            if (cnt <= 0) continue;
            if (c0 < 0) c0 = col_first[I];
            const int64_t off = regrid_lane_offset(col_first[I], static_cast<int32_t>(c0), nx, true);
            if (off < 0) return sp;
            end = off + cnt > end ? off + cnt : end;
        }
    } else {
        for (int32_t I = I0; I < I1; ++I) {
            const int64_t cnt = static_cast<int64_t>(col_ptr[I + 1]) - col_ptr[I];
            if (cnt <= 0) continue;
            if (c0 < 0 || col_first[I] < c0) c0 = col_first[I];
        }
        for (int32_t I = I0; I < I1 && c0 >= 0; ++I) {
            const int64_t cnt = static_cast<int64_t>(col_ptr[I + 1]) - col_ptr[I];
            if (cnt <= 0) continue;
            const int64_t e = col_first[I] - c0 + cnt;
            end = e > end ? e : end;
        }
    }
    if (c0 < 0 || c0 >= nx || end > INT32_MAX) return sp;
    sp.c0 = static_cast<int32_t>(c0);
    sp.width = static_cast<int32_t>(end);
    return sp;
}

// the widest span over the tiles of a call
XMHW_REGRID_FN int32_t regrid_max_width(const int32_t* col_first, const int32_t* col_ptr, int32_t mx, int32_t nx, bool periodic) {
    int32_t most = 0;
    for (int32_t I0 = 0; I0 < mx; I0 += kRegridTile) {
        const int32_t w = regrid_tile_span(col_first, col_ptr, mx, nx, periodic, I0).width;
        most = w > most ? w : most;
    }
    return most;
}

// the LDS slot of entry k of a lane's run in source row r of the tile; -1 outside the tile
XMHW_REGRID_FN int32_t regrid_lds_slot(int32_t rows, int32_t width, int32_t r, int32_t off, int32_t k) {
    if (rows < 0 || width < 0 || r < 0 || r >= rows || off < 0 || k < 0 || static_cast<int64_t>(off) + k >= width) return -1;
    const int64_t s = static_cast<int64_t>(r) * width + off + k;
    return s < kRegridLdsDwords ? static_cast<int32_t>(s) : -1;
}

// does one step of the largest footprint fit the LDS tile?  (an empty footprint does not: there is nothing to stage)
XMHW_REGRID_FN bool regrid_fits(int32_t max_rows, int32_t max_width, int32_t nx, bool periodic) {
    if (max_rows < 1 || max_width < 1 || nx < 1 || (!periodic && max_width > nx)) return false;
    return static_cast<int64_t>(max_rows) * max_width <= kRegridLdsDwords;
}

// The automatic choice among the calls that fit, as measured: the staged path wins where the lanes of a
// tile read disjoint, strided runs -- two source columns per lane and more, which the direct path loads uncoalesced -- and
// the tile is small enough for many workgroups per CU, kRegridAutoDwords at most; it loses where footprints overlap, where
// many lanes share a column and where the tile is large.  `lanes` = the destination columns of the widest tile.
XMHW_REGRID_FN bool regrid_auto_staged(int32_t max_rows, int32_t max_width, int32_t lanes) {
    return lanes >= 1 && static_cast<int64_t>(max_rows) * max_width <= kRegridAutoDwords &&
           static_cast<int64_t>(max_width) >= 2 * static_cast<int64_t>(lanes);
}

// the path of a call: `variant` 0 = automatic, 1 = direct, 2 = staged where it fits
XMHW_REGRID_FN int32_t regrid_class(int32_t max_rows, int32_t max_width, int32_t lanes, int32_t nx, bool periodic, int32_t variant) {
    if (variant < 0 || variant > 2 || nx < 1) return kRegridNone;
    if (variant == 1 || !regrid_fits(max_rows, max_width, nx, periodic)) return kRegridDirect;
    return variant == 2 || regrid_auto_staged(max_rows, max_width, lanes) ? kRegridStaged : kRegridDirect;
}

// the chunks of `per` steps that cover nt steps, and chunk k of them: steps *t0 .. *t1 - 1 (empty outside)
XMHW_REGRID_FN int64_t regrid_chunks(int64_t nt, int64_t per) { return nt > 0 && per > 0 ? (nt + per - 1) / per : 0; }
XMHW_REGRID_FN void regrid_chunk(int64_t k, int64_t nt, int64_t per, int64_t* t0, int64_t* t1) {
    *t0 = *t1 = 0;
    if (k < 0 || k >= regrid_chunks(nt, per)) return;
    const int64_t a = k * per, b = a + per;
    *t0 = a;
    *t1 = b < nt ? b : nt;
}

// The automatic chunk: a chunk carries nothing over, so short chunks cost a workgroup's start and its table reads and no
// more.  About 256 samples per lane and chunk (`work` = the largest footprint, rows x columns), 4 steps at least, 64 at
// most, in multiples of the 4 steps the direct path requests together; a grid too small to fill the chip with such chunks
// splits the steps until about 2048 workgroups exist.
static inline int64_t regrid_auto_chunk(int64_t nt, int64_t workgroups, int64_t work) {
    if (nt <= 0) return 1;
    int64_t cap = 256 / (work > 0 ? work : 1);
    cap = cap < 4 ? 4 : cap > 64 ? 64 : cap;
    return stage_auto_block(nt, workgroups > 0 ? workgroups : 1, nt, cap, 4);
}

}  // namespace xmhw
