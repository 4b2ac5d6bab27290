// halo_tile.h -- the index arithmetic of spatial_correlation() (kernels_spatialcorr.hip): a workgroup owns
// a tile of `rows` grid rows x 64 longitudes and stages, per step, the tile plus the halo its offsets reach in LDS.  Plain
// integer code without a device type: the kernel, the launcher (the LDS size) and a host program (tests/c/halo_tile.cpp,
// against a brute-force lookup) compile the same functions.  Every function checks what it is given against the tile and
// the grid and answers -1 for anything outside, whatever the offset table holds.
//
//   the tile      workgroup w of tiles_x x tiles_y: grid rows j0 .. j0 + rows - 1, columns i0 .. i0 + 63 (the last tile of
//                 an axis hangs over the grid; its lanes own nothing)
//   the box       of a group of offsets: the bounding box [dj0, dj1] x [di0, di1] of its (dj, di) and of (0, 0), each
//                 offset clamped to the reach of 32 points: the halo is what the call's offsets reach, not the cap
//   the LDS tile  H = rows + dj1 - dj0 rows of W = 64 + di1 - di0 dwords, slot (r, c) = r * W + c: tile row r is grid row
//                 j0 + dj0 + r, tile column c is grid column i0 + di0 + c (taken mod nx across a periodic seam)
//   a lane        (rr, cc) of the tile reads, for the offset (dj, di), slot (rr + dj - dj0, cc + di - di0): a wave is one
//                 tile row, so its 64 lanes read 64 consecutive dwords
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XMHW_HALO_FN __host__ __device__ static inline
#else
#define XMHW_HALO_FN static inline
#endif

namespace xmhw {

constexpr int kHaloCols = 64;                        // longitudes of a tile: one wave
constexpr int kHaloReach = 32;                       // |dj|, |di| at most

struct HaloBox {
    int32_t dj0, dj1, di0, di1;                      // inclusive; dj0 <= 0 <= dj1, di0 <= 0 <= di1
};

XMHW_HALO_FN int32_t halo_clamp(int32_t d) { return d < -kHaloReach ? -kHaloReach : d > kHaloReach ? kHaloReach : d; }

// the tiles of a grid axis
XMHW_HALO_FN int64_t halo_tiles_x(int32_t nx) { return nx > 0 ? (static_cast<int64_t>(nx) + kHaloCols - 1) / kHaloCols : 0; }
XMHW_HALO_FN int64_t halo_tiles_y(int32_t ny, int32_t rows) {
    return ny > 0 && rows > 0 ? (static_cast<int64_t>(ny) + rows - 1) / rows : 0;
}

// the origin (j0, i0) of workgroup w, row-major over tiles_y x tiles_x; false if w is no tile of the grid
XMHW_HALO_FN bool halo_origin(int64_t w, int32_t ny, int32_t nx, int32_t rows, int32_t* j0, int32_t* i0) {
    const int64_t tx = halo_tiles_x(nx), ty = halo_tiles_y(ny, rows);
    if (w < 0 || tx <= 0 || w >= tx * ty) return false;
    *j0 = static_cast<int32_t>(w / tx) * rows;
    *i0 = static_cast<int32_t>(w % tx) * kHaloCols;
    return true;
}

// the box of `count` offsets djdi[2 * e], djdi[2 * e + 1]
XMHW_HALO_FN HaloBox halo_box(const int32_t* djdi, int32_t count) {
    HaloBox b = {0, 0, 0, 0};
    for (int32_t e = 0; e < count; ++e) {
        const int32_t dj = halo_clamp(djdi[2 * e]), di = halo_clamp(djdi[2 * e + 1]);
        b.dj0 = dj < b.dj0 ? dj : b.dj0;
        b.dj1 = dj > b.dj1 ? dj : b.dj1;
        b.di0 = di < b.di0 ? di : b.di0;
        b.di1 = di > b.di1 ? di : b.di1;
    }
    return b;
}

XMHW_HALO_FN bool halo_box_ok(const HaloBox& b) {
    return b.dj0 >= -kHaloReach && b.dj0 <= 0 && b.dj1 >= 0 && b.dj1 <= kHaloReach && b.di0 >= -kHaloReach && b.di0 <= 0 &&
           b.di1 >= 0 && b.di1 <= kHaloReach;
}
XMHW_HALO_FN int32_t halo_height(const HaloBox& b, int32_t rows) { return rows + b.dj1 - b.dj0; }
XMHW_HALO_FN int32_t halo_width(const HaloBox& b) { return kHaloCols + b.di1 - b.di0; }
XMHW_HALO_FN int32_t halo_slots(const HaloBox& b, int32_t rows) { return halo_height(b, rows) * halo_width(b); }

// the LDS slot of tile (row r, column c), -1 outside the tile
XMHW_HALO_FN int32_t halo_slot(const HaloBox& b, int32_t rows, int32_t r, int32_t c) {
    if (!halo_box_ok(b) || rows < 1 || r < 0 || r >= halo_height(b, rows) || c < 0 || c >= halo_width(b)) return -1;
    return r * halo_width(b) + c;
}

// the grid point j * nx + i behind tile (r, c) of the tile at (j0, i0): across a periodic seam the column wraps, a point
// outside the grid (and any r, c outside the tile) is -1
XMHW_HALO_FN int64_t halo_point(const HaloBox& b, int32_t rows, int32_t j0, int32_t i0, int32_t r, int32_t c, int32_t ny,
                                int32_t nx, bool periodic) {
    if (halo_slot(b, rows, r, c) < 0 || ny < 1 || nx < 1 || j0 < 0 || i0 < 0) return -1;
    const int64_t j = static_cast<int64_t>(j0) + b.dj0 + r;
    int64_t i = static_cast<int64_t>(i0) + b.di0 + c;
    if (j < 0 || j >= ny) return -1;
    if (i < 0 || i >= nx) {
        if (!periodic) return -1;
        i %= nx;
        if (i < 0) i += nx;
    }
    return j * nx + i;
}

// the slot lane (rr, cc) of the tile reads for the offset (dj, di); -1 if the lane is no lane of the tile or the offset
// leaves the box
XMHW_HALO_FN int32_t halo_read_slot(const HaloBox& b, int32_t rows, int32_t rr, int32_t cc, int32_t dj, int32_t di) {
    if (rr < 0 || rr >= rows || cc < 0 || cc >= kHaloCols) return -1;
    if (dj < b.dj0 || dj > b.dj1 || di < b.di0 || di > b.di1) return -1;
    return halo_slot(b, rows, rr + dj - b.dj0, cc + di - b.di0);
}

// the grid point lane (rr, cc) owns, -1 if it hangs over the grid (never wrapped: a lane past the seam owns nothing)
XMHW_HALO_FN int64_t halo_own_point(int32_t rows, int32_t j0, int32_t i0, int32_t rr, int32_t cc, int32_t ny, int32_t nx) {
    if (rr < 0 || rr >= rows || cc < 0 || cc >= kHaloCols || j0 < 0 || i0 < 0) return -1;
    const int64_t j = static_cast<int64_t>(j0) + rr, i = static_cast<int64_t>(i0) + cc;
    return j < ny && i < nx ? j * nx + i : -1;
}

}  // namespace xmhw
