// The index arithmetic of coarsen() (xmhw_amd/csrc/coarsen_index.h) and its chunk rule (stage_blocks.h) against brute
// force: for grids of 1 to 20 points per axis, factors of 1 to 9 and both the floor and the ceil coarse grid, a table of
// the fine grid is built point by point -- which coarse cell owns the point, written without any of the header's
// arithmetic (a running counter per axis) --, and every block the header answers is walked over that table: every point
// of the block must belong to the cell, and every point of the cell's count must be reached.  The table has exactly the
// size of the grid, so an origin or an extent outside it stops the program under AddressSanitizer.  The alignment class
// is compared with an address-by-address check of every load a lane would make, for every class; the chunks with a
// window-by-window cover.  Prints the number of checks made; tests/test_host_coarsen_index.py builds this with
// -fsanitize=address,undefined and asserts a floor on it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/coarsen_index.h"
#include "../../xmhw_amd/csrc/stage_blocks.h"

using namespace xmhw;

static long long checks = 0;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        ++checks;                                                                        \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

// owner[j * nx + i] = the coarse cell of the fine point, -1 where the coarse grid does not reach; by running counters
static std::vector<long long> owners(int ny, int nx, int fy, int fx, int ncy, int ncx) {
    std::vector<long long> owner(static_cast<size_t>(ny) * nx, -1);
    int J = 0, rj = 0;
    for (int j = 0; j < ny; ++j) {
        int I = 0, ri = 0;
        for (int i = 0; i < nx; ++i) {
            if (J < ncy && I < ncx) owner.at(static_cast<size_t>(j) * nx + i) = static_cast<long long>(J) * ncx + I;
            if (++ri == fx) { ri = 0; ++I; }
        }
        if (++rj == fy) { rj = 0; ++J; }
    }
    return owner;
}

static void check_blocks() {
    for (int ny = 1; ny <= 20; ++ny)
        for (int nx = 1; nx <= 20; ++nx)
            for (int fy = 1; fy <= 9; ++fy)
                for (int fx = 1; fx <= 9; ++fx)
                    for (int up = 0; up < 2; ++up) {
                        const int ncy = coarsen_cells(ny, fy, up != 0), ncx = coarsen_cells(nx, fx, up != 0);
                        int by = 0, bx = 0;                          // the cells by brute force
                        for (int j = 0; j < ny; j += fy) by += up || j + fy <= ny;
                        for (int i = 0; i < nx; i += fx) bx += up || i + fx <= nx;
                        CHECK(ncy == by && ncx == bx);
                        CHECK(coarsen_grid_ok(ny, nx, fy, fx, ncy, ncx));
                        CHECK(!coarsen_grid_ok(ny, nx, fy, fx, coarsen_cells(ny, fy, true) + 1, ncx));
                        CHECK(!coarsen_grid_ok(ny, nx, fy, fx, ncy, coarsen_cells(nx, fx, true) + 1));
                        const std::vector<long long> owner = owners(ny, nx, fy, fx, ncy, ncx);
                        std::vector<int> reached(static_cast<size_t>(ny) * nx, 0);
                        const long long cells = static_cast<long long>(ncy) * ncx;
                        for (long long c = -1; c <= cells; ++c) {
                            const CoarsenBlock b = coarsen_block(c, ny, nx, fy, fx, ncy, ncx);
                            if (c < 0 || c >= cells) {               // a lane without a cell: nothing
                                CHECK(b.h == 0 && b.w == 0);
                                continue;
                            }
                            CHECK(b.h >= 1 && b.h <= fy && b.w >= 1 && b.w <= fx);
                            CHECK(up || (b.h == fy && b.w == fx));   // a floor grid has whole blocks only
                            for (int r = 0; r < b.h; ++r)
                                for (int k = 0; k < b.w; ++k) {
                                    const size_t p = static_cast<size_t>(b.j0 + r) * nx + (b.i0 + k);
                                    CHECK(owner.at(p) == c);
                                    ++reached.at(p);
                                }
                        }
                        for (size_t p = 0; p < owner.size(); ++p) CHECK(reached[p] == (owner[p] >= 0 ? 1 : 0));
                    }
    // outside: no block
    CHECK(coarsen_block(0, 4, 4, 0, 1, 1, 1).h == 0 && coarsen_block(0, 4, 4, 1, 1, 5, 1).h == 0);
    CHECK(coarsen_block(0, -1, 4, 1, 1, 1, 1).w == 0 && coarsen_cells(-3, 2, true) == 0 && coarsen_cells(3, 0, true) == 0);
}

// every load a lane of the class would make, address by address: is it a multiple of its width?
static bool loads_aligned(unsigned long long ts, unsigned long long wi, long long ld, int nx, int isz, int fx) {
    const long long ab = fx * isz > 16 ? 16 : fx * isz, wb = fx * 4 > 16 ? 16 : fx * 4;
    for (int t = 0; t < 3; ++t)
        for (int j = 0; j < 3; ++j)
            for (int I = 0; (I + 1) * fx <= nx; ++I) {
                if ((ts + static_cast<unsigned long long>((t * ld + static_cast<long long>(j) * nx + I * fx) * isz)) % ab) return false;
                if ((wi + static_cast<unsigned long long>((static_cast<long long>(j) * nx + I * fx) * 4)) % wb) return false;
            }
    return true;
}

static void check_classes() {
    bool seen[kCoarsenClasses] = {false, false, false, false, false, false};
    for (int isz = 4; isz <= 8; isz += 4)
        for (int fx = 1; fx <= 9; ++fx)
            for (int nx = fx; nx <= 20; ++nx)
                for (long long ld = static_cast<long long>(3) * nx; ld <= 3 * nx + 4; ++ld)
                    for (unsigned long long ts = 4096; ts < 4096 + 32; ts += isz)
                        for (unsigned long long wi = 8192; wi < 8192 + 16; wi += 4) {
                            const int32_t k = coarsen_class(ts, wi, ld, nx, isz, fx, false, false);
                            seen[k] = true;
                            if (fx != 1 && fx != 2 && fx != 4) {
                                CHECK(k == kCoarsenGeneric);
                            } else if (fx == 1) {
                                CHECK(k == kCoarsenFx1);
                            } else {
                                const bool wide = loads_aligned(ts, wi, ld, nx, isz, fx);
                                CHECK(k == (fx == 2 ? (wide ? kCoarsenFx2Wide : kCoarsenFx2) : (wide ? kCoarsenFx4Wide : kCoarsenFx4)));
                            }
                            const int32_t narrow = coarsen_class(ts, wi, ld, nx, isz, fx, true, false);
                            CHECK(narrow == (fx == 1 ? kCoarsenFx1 : fx == 2 ? kCoarsenFx2 : fx == 4 ? kCoarsenFx4 : kCoarsenGeneric));
                            CHECK(coarsen_class(ts, wi, ld, nx, isz, fx, false, true) == kCoarsenGeneric);
                        }
    for (bool s : seen) CHECK(s);
    CHECK(coarsen_class(4096, 8192, 16, 16, 2, 2, false, false) == kCoarsenGeneric);     // no sample type of 2 bytes
}

static void check_chunks() {
    for (int ns = 0; ns <= 40; ++ns)
        for (int per = 0; per <= 45; ++per) {
            const long long chunks = coarsen_chunks(ns, per);
            CHECK(chunks == (ns > 0 && per > 0 ? (ns + per - 1) / per : 0));
            std::vector<int> covered(static_cast<size_t>(ns), 0);
            for (long long k = -1; k <= chunks; ++k) {
                int32_t s0 = -7, s1 = -7;
                coarsen_chunk(k, ns, per, &s0, &s1);
                if (k < 0 || k >= chunks) {
                    CHECK(s0 == s1);
                    continue;
                }
                CHECK(s0 < s1 && s1 - s0 <= per && s1 <= ns);
                for (int s = s0; s < s1; ++s) ++covered.at(static_cast<size_t>(s));
            }
            for (int c : covered) CHECK(c == (per > 0 ? 1 : 0));     // every window once (no chunk of no windows)
        }
    // the automatic chunk: about 64 lines x steps of requests per lane where the grid fills the chip, one window at least,
    // never more windows than there are; a small grid splits the windows until about 2048 workgroups exist
    CHECK(coarsen_auto_chunk(14610, 259200, 2, 1) == 32);            // ceil(14610 / ceil(14610 / 32))
    CHECK(coarsen_auto_chunk(14610, 64800, 4, 1) == 16);
    CHECK(coarsen_auto_chunk(487, 1036800, 1, 30) == 2);             // 64 / 30 = 2 windows a chunk
    CHECK(coarsen_auto_chunk(100, 256, 1, 1) == 1);                  // 2048 workgroups of one window would exist: 100 do
    CHECK(coarsen_auto_chunk(0, 256, 1, 1) == 1 && coarsen_auto_chunk(5, 0, 1, 1) >= 1);
    for (long long ns = 1; ns <= 300; ns += 13)
        for (long long cells = 1; cells <= 1 << 20; cells *= 4)
            for (long long rows = 1; rows <= 64; rows *= 2) {
                const long long per = coarsen_auto_chunk(ns, cells, rows, 3);
                CHECK(per >= 1 && per <= ns);
            }
}

int main() {
    check_blocks();
    check_classes();
    check_chunks();
    std::printf("%lld\n", checks);
    return 0;
}
