// The index arithmetic of spatial_correlation() (xmhw_amd/csrc/halo_tile.h) against a brute-force lookup: for grids from
// 1 x 1 to 9 x 200, both seam settings, both tile shapes, every tile and the offset boxes whose four bounds run over
// {0, 1, 32} (no halo, one point, the cap) -- on the six grids of up to 2 x 33 over {0, 1, 7, 31, 32}: a sample of the
// 33^4 boxes up to the cap, which cannot all be walked in a test --, the tile is filled slot by slot as the kernel fills
// it and read lane by lane as the kernel reads it, and both are compared with a table of the grid that is built without
// any of the header's arithmetic (every wrapped copy of a column is written out).  The arrays have exactly the size the header states, so an
// index outside them stops the program under AddressSanitizer.  Prints the number of checks made;
// tests/test_host_halo_tile.py builds this with -fsanitize=address,undefined and asserts a floor on it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/halo_tile.h"

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

// the grid by brute force: point[(j + PAD) * width + (i + PAD)] for j, i in [-PAD, n + PAD), -1 outside the grid; on a
// periodic grid every copy of column i at i + m * nx is written out
struct Lookup {
    static constexpr int PAD = 140;                  // a tile hangs over by up to 63 columns, a halo reaches 32 more
    int ny, nx, width;
    std::vector<long long> point;
    Lookup(int ny_, int nx_, bool periodic) : ny(ny_), nx(nx_), width(nx_ + 2 * PAD), point(static_cast<size_t>(ny_ + 2 * PAD) * (nx_ + 2 * PAD), -1) {
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                for (int m = periodic ? -PAD : 0; m <= (periodic ? PAD : 0); ++m) {
                    const long long col = i + static_cast<long long>(m) * nx;
                    if (col >= -PAD && col < nx + PAD) at(j, static_cast<int>(col)) = static_cast<long long>(j) * nx + i;
                }
    }
    long long& at(int j, int i) { return point.at(static_cast<size_t>(j + PAD) * width + (i + PAD)); }
};

static void check_boxes() {
    // the box of a table: the extremes of its offsets and of (0, 0), clamped at the reach
    const int32_t t1[] = {3, -2, -1, 5, 0, 0, 3, -2};
    HaloBox b = halo_box(t1, 4);
    CHECK(b.dj0 == -1 && b.dj1 == 3 && b.di0 == -2 && b.di1 == 5);
    const int32_t t2[] = {2, 4};
    b = halo_box(t2, 1);
    CHECK(b.dj0 == 0 && b.dj1 == 2 && b.di0 == 0 && b.di1 == 4);
    const int32_t t3[] = {-1000, 77, 33, -33};
    b = halo_box(t3, 2);
    CHECK(b.dj0 == -32 && b.dj1 == 32 && b.di0 == -32 && b.di1 == 32 && halo_box_ok(b));
    b = halo_box(t3, 0);
    CHECK(b.dj0 == 0 && b.dj1 == 0 && b.di0 == 0 && b.di1 == 0);
    for (int dj = -kHaloReach; dj <= kHaloReach; ++dj)
        for (int di = -kHaloReach; di <= kHaloReach; ++di) {
            const int32_t one[] = {dj, di};
            b = halo_box(one, 1);
            CHECK(b.dj0 == (dj < 0 ? dj : 0) && b.dj1 == (dj > 0 ? dj : 0) && b.di0 == (di < 0 ? di : 0) &&
                  b.di1 == (di > 0 ? di : 0) && halo_box_ok(b));
        }
    const HaloBox bad = {1, 2, 0, 0};
    CHECK(!halo_box_ok(bad) && halo_slot(bad, 4, 0, 0) == -1);
}

static void check_grid(int ny, int nx, bool periodic, int rows) {
    Lookup grid(ny, nx, periodic);
    const long long tiles = halo_tiles_x(nx) * halo_tiles_y(ny, rows);
    // every grid point is owned by exactly one lane of one tile
    std::vector<int> owners(static_cast<size_t>(ny) * nx, 0);
    int32_t j0 = -1, i0 = -1;
    CHECK(!halo_origin(-1, ny, nx, rows, &j0, &i0) && !halo_origin(tiles, ny, nx, rows, &j0, &i0));
    for (long long w = 0; w < tiles; ++w) {
        CHECK(halo_origin(w, ny, nx, rows, &j0, &i0));
        CHECK(j0 >= 0 && j0 < ny && j0 % rows == 0 && i0 >= 0 && i0 < nx && i0 % kHaloCols == 0);
        for (int rr = 0; rr < rows; ++rr)
            for (int cc = 0; cc < kHaloCols; ++cc) {
                const long long p = halo_own_point(rows, j0, i0, rr, cc, ny, nx);
                const bool inside = j0 + rr < ny && i0 + cc < nx;
                CHECK(p == (inside ? static_cast<long long>(j0 + rr) * nx + (i0 + cc) : -1));
                if (p >= 0) ++owners.at(static_cast<size_t>(p));
            }
        CHECK(halo_own_point(rows, j0, i0, rows, 0, ny, nx) == -1 && halo_own_point(rows, j0, i0, 0, kHaloCols, ny, nx) == -1 &&
              halo_own_point(rows, j0, i0, -1, 0, ny, nx) == -1);
    }
    for (int v : owners) CHECK(v == 1);
    // every grid takes the 81 boxes with bounds in {0, 1, 32}; the grids of up to 2 x 33 the 625 with 7 and 31 too (tile
    // widths such as 64 + 7 and 64 + 31 + 1); all 33^4 boxes up to the cap are out of reach
    const bool small = ny <= 2 && nx <= 33;
    const std::vector<int> bounds = small ? std::vector<int>{0, 1, 7, 31, kHaloReach} : std::vector<int>{0, 1, kHaloReach};
    for (int a : bounds)
        for (int b : bounds)
            for (int c : bounds)
                for (int d : bounds) {
                    const HaloBox box = {-a, b, -c, d};
                    const int H = halo_height(box, rows), W = halo_width(box), S = halo_slots(box, rows);
                    CHECK(H == rows + a + b && W == kHaloCols + c + d && S == H * W);
                    // outside the tile: no slot, no point
                    CHECK(halo_slot(box, rows, -1, 0) == -1 && halo_slot(box, rows, H, 0) == -1 &&
                          halo_slot(box, rows, 0, -1) == -1 && halo_slot(box, rows, 0, W) == -1);
                    for (long long w = 0; w < tiles; ++w) {
                        halo_origin(w, ny, nx, rows, &j0, &i0);
                        CHECK(halo_point(box, rows, j0, i0, H, 0, ny, nx, periodic) == -1 &&
                              halo_point(box, rows, j0, i0, 0, W, ny, nx, periodic) == -1);
                        // the tile as the kernel fills it: every slot once, the point behind it from the lookup
                        std::vector<long long> tile(static_cast<size_t>(S), -2);
                        for (int r = 0; r < H; ++r)
                            for (int col = 0; col < W; ++col) {
                                const int s = halo_slot(box, rows, r, col);
                                CHECK(s >= 0 && s < S && tile.at(static_cast<size_t>(s)) == -2);
                                const long long p = halo_point(box, rows, j0, i0, r, col, ny, nx, periodic);
                                CHECK(p == grid.at(j0 - a + r, i0 - c + col));
                                tile.at(static_cast<size_t>(s)) = p;
                            }
                        // ... and as the kernel reads it: a lane finds the partner of its own point at every offset
                        const int djs[] = {-a, 0, b}, dis[] = {-c, 0, d};
                        for (int rr = 0; rr < rows; ++rr)
                            for (int cc = 0; cc < kHaloCols; ++cc)
                                for (int dj : djs)
                                    for (int di : dis) {
                                        const int s = halo_read_slot(box, rows, rr, cc, dj, di);
                                        CHECK(s >= 0 && s < S);
                                        CHECK(tile.at(static_cast<size_t>(s)) == grid.at(j0 + rr + dj, i0 + cc + di));
                                    }
                        // an offset that leaves the box, a lane that is none
                        CHECK(halo_read_slot(box, rows, 0, 0, b + 1, 0) == -1 && halo_read_slot(box, rows, 0, 0, -a - 1, 0) == -1 &&
                              halo_read_slot(box, rows, 0, 0, 0, d + 1) == -1 && halo_read_slot(box, rows, 0, 0, 0, -c - 1) == -1 &&
                              halo_read_slot(box, rows, rows, 0, 0, 0) == -1 && halo_read_slot(box, rows, 0, kHaloCols, 0, 0) == -1);
                    }
                }
}

int main() {
    check_boxes();
    const int nys[] = {1, 2, 3, 4, 5, 8, 9}, nxs[] = {1, 2, 33, 64, 65, 130, 200};
    for (int ny : nys)
        for (int nx : nxs)
            for (int periodic = 0; periodic < 2; ++periodic)
                for (int rows : {4, 8}) check_grid(ny, nx, periodic != 0, rows);
    std::printf("%lld\n", checks);
    return 0;
}
