// coarsen_index.h -- the index arithmetic of coarsen() (kernels_coarsen.hip): a lane owns one coarse cell
// and walks the block of fy x fx fine points behind it over the steps of a window.  Plain integer code without a device
// type, as halo_tile.h: the kernel, the launcher and a host program (tests/c/coarsen_index.cpp, against a brute-force
// table) compile the same functions.  Every function checks what it is given and answers with an empty block, class 0
// or an empty chunk for anything outside.
//
//   the cell      flat index c = J * ncx + I of the ncy x ncx coarse grid, ncy <= ceil(ny / fy), ncx <= ceil(nx / fx):
//                 lanes are consecutive c, so only the last workgroup has lanes without a cell
//   the block     fine rows J * fy .. J * fy + h - 1 and columns I * fx .. I * fx + w - 1 with h = min(fy, ny - J * fy)
//                 and w = min(fx, nx - I * fx): a block that hangs over the grid holds its in-grid points only
//   the class     which instantiation reads the samples: a lane's fx samples of a row in one load of its full width
//                 where every lane of every row and step is aligned for it, dword (one sample) loads otherwise
//   the chunk     workgroups along grid.y take chunks of consecutive windows
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XMHW_COARSEN_FN __host__ __device__ static inline
#else
#define XMHW_COARSEN_FN static inline
#endif

namespace xmhw {

constexpr int kCoarsenMaxVolume = 4096;              // fy * fx * (steps of the longest window) at most

// the instantiations of the kernel
enum CoarsenClass : int32_t {
    kCoarsenGeneric = 0,                             // any fx: a run-time column loop, one sample per load
    kCoarsenFx1 = 1,                                 // fx == 1: one sample per row and step
    kCoarsenFx2 = 2,                                 // fx == 2, two loads of one sample
    kCoarsenFx2Wide = 3,                             // fx == 2, one load of two samples
    kCoarsenFx4 = 4,                                 // fx == 4, four loads of one sample
    kCoarsenFx4Wide = 5,                             // fx == 4, one load of four samples (two of 16 bytes for float64)
    kCoarsenClasses = 6
};

struct CoarsenBlock {
    int32_t j0, i0;                                  // the first fine row and column
    int32_t h, w;                                    // the in-grid rows and columns: 0 x 0 for a lane without a cell
};

// the cells of an axis: ceil (a partial last block is kept) or floor (it is dropped)
XMHW_COARSEN_FN int32_t coarsen_cells(int32_t n, int32_t f, bool ceil) {
    if (n < 0 || f < 1) return 0;
    return static_cast<int32_t>(ceil ? (static_cast<int64_t>(n) + f - 1) / f : n / f);
}

// is ncy x ncx a coarse grid of ny x nx under (fy, fx)?  (0 cells on an axis is one: nothing is computed)
XMHW_COARSEN_FN bool coarsen_grid_ok(int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy, int32_t ncx) {
    return ny >= 0 && nx >= 0 && fy >= 1 && fx >= 1 && ncy >= 0 && ncx >= 0 && ncy <= coarsen_cells(ny, fy, true) &&
           ncx <= coarsen_cells(nx, fx, true);
}

// flat cell -> the origin and the in-grid extents of its block
XMHW_COARSEN_FN CoarsenBlock coarsen_block(int64_t c, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy,
                                           int32_t ncx) {
    CoarsenBlock b = {0, 0, 0, 0};
    if (!coarsen_grid_ok(ny, nx, fy, fx, ncy, ncx) || c < 0 || c >= static_cast<int64_t>(ncy) * ncx) return b;
    const int64_t j0 = (c / ncx) * fy, i0 = (c % ncx) * fx;       // < ny, < nx: the cell is one of the coarse grid
    b.j0 = static_cast<int32_t>(j0);
    b.i0 = static_cast<int32_t>(i0);
    b.h = static_cast<int32_t>(ny - j0 < fy ? ny - j0 : fy);
    b.w = static_cast<int32_t>(nx - i0 < fx ? nx - i0 : fx);
    return b;
}

// the bytes a wide load of `fx` items of `itemsize` bytes must be aligned to: the lane's full width, 16 at most
XMHW_COARSEN_FN int64_t coarsen_wide_bytes(int32_t fx, int32_t itemsize) {
    const int64_t full = static_cast<int64_t>(fx) * itemsize;
    return full > 16 ? 16 : full;
}

// The class of a call.  A lane reads its samples at ts + ((t * ld + j * nx + I * fx) * itemsize) and its weights at
// wi + (j * nx + I * fx) * 4: the wide form is taken when the two addresses, ld * itemsize, nx * itemsize and nx * 4 keep
// every one of them a multiple of the load's width.  `force_narrow` keeps the loads at one sample; `force_generic` picks
// the run-time column loop whatever fx is (tests and measurements).
XMHW_COARSEN_FN int32_t coarsen_class(uint64_t ts_addr, uint64_t wi_addr, int64_t ld, int32_t nx, int32_t itemsize,
                                      int32_t fx, bool force_narrow, bool force_generic) {
    if (force_generic || (fx != 1 && fx != 2 && fx != 4) || (itemsize != 4 && itemsize != 8) || ld < 0 || nx < 0)
        return kCoarsenGeneric;
    if (fx == 1) return kCoarsenFx1;
    const uint64_t ab = static_cast<uint64_t>(coarsen_wide_bytes(fx, itemsize));
    const uint64_t wb = static_cast<uint64_t>(coarsen_wide_bytes(fx, 4));
    const bool wide = !force_narrow && ts_addr % ab == 0 && (static_cast<uint64_t>(ld) * itemsize) % ab == 0 &&
                      (static_cast<uint64_t>(nx) * itemsize) % ab == 0 && wi_addr % wb == 0 &&
                      (static_cast<uint64_t>(nx) * 4) % wb == 0;
    return fx == 2 ? (wide ? kCoarsenFx2Wide : kCoarsenFx2) : (wide ? kCoarsenFx4Wide : kCoarsenFx4);
}

// the chunks of `per` windows that cover ns windows, and chunk k of them: windows *s0 .. *s1 - 1 (empty outside)
XMHW_COARSEN_FN int64_t coarsen_chunks(int32_t ns, int32_t per) {
    return ns > 0 && per > 0 ? (static_cast<int64_t>(ns) + per - 1) / per : 0;
}
XMHW_COARSEN_FN void coarsen_chunk(int64_t k, int32_t ns, int32_t per, int32_t* s0, int32_t* s1) {
    *s0 = *s1 = 0;
    if (k < 0 || k >= coarsen_chunks(ns, per)) return;
    const int64_t a = k * per, b = a + per;
    *s0 = static_cast<int32_t>(a);
    *s1 = static_cast<int32_t>(b < ns ? b : ns);
}

}  // namespace xmhw
