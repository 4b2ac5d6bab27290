// The index arithmetic of regrid() (xmhw_amd/csrc/regrid_index.h) against brute force.  Column tables are drawn from a
// small generator of its own (monotone or not, strided, repeated, empty runs, runs that cross a periodic seam, a run as
// long as the grid) for destination widths of 1 to 600 columns and source grids of 1 to 700.  For every tile: the tile
// map is compared with a running counter; a table `held` of exactly the span's width is filled slot by slot with the
// source column regrid_source_col() names, and every entry of every lane's run is then looked up through
// regrid_lane_offset() / regrid_lds_slot() and must hold the column (col_first + k) mod nx that the definition names --
// the tables have exactly the sizes the kernel allocates, so a slot or a column outside them stops the program under
// AddressSanitizer.  The span is the smallest that holds every run from its start.  The fit test and the class are
// compared with their definition, the layout of the packed table with a running offset, the chunks with a step-by-step
// cover.  Prints the number of checks made; tests/test_host_regrid_index.py builds this with
// -fsanitize=address,undefined and asserts a floor on it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/regrid_index.h"

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

static unsigned long long state = 88172645463325252ull;
static int draw(int n) {                                 // 0 .. n - 1 (xorshift)
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return static_cast<int>((state >> 11) % static_cast<unsigned long long>(n));
}

struct Table {
    int nx = 1;
    bool periodic = false;
    std::vector<int32_t> first, ptr;
};

// kind 0: random monotone, 1: refining (repeated firsts), 2: strided, 3: unordered; runs of 0 .. 64, inside the grid
static Table make(int mx, int nx, bool periodic, int kind) {
    Table t;
    t.nx = nx;
    t.periodic = periodic;
    t.ptr.push_back(0);
    const int lengths[9] = {0, 1, 2, 3, 4, 5, 8, 17, 64};
    int at = draw(nx);
    const int stride = 1 + draw(8), share = 2 + draw(3);
    for (int I = 0; I < mx; ++I) {
        int cnt = kind == 1 ? 1 + (I % share == 0) : kind == 2 ? stride + draw(2) : lengths[draw(9)];
        if (kind == 3) at = draw(nx);
        else if (kind == 1) at += I % share == 0;
        else at += kind == 2 ? stride : draw(4);
        if (I == mx / 2 && draw(2)) cnt = nx;            // a run as long as the grid
        cnt = cnt > kRegridMaxRun ? kRegridMaxRun : cnt;
        cnt = cnt > nx ? nx : cnt;
        int f;
        if (periodic) {
            f = at % nx;
        } else {
            f = at % nx;
            if (f + cnt > nx) f = nx - cnt;              // kept inside the grid
        }
        t.first.push_back(f);
        t.ptr.push_back(t.ptr.back() + cnt);
    }
    return t;
}

static void check_tiles_and_spans() {
    const int widths[] = {1, 2, 7, 63, 64, 65, 130, 255, 256, 257, 511, 600};
    const int grids[] = {1, 2, 3, 5, 64, 65, 100, 257, 700};
    for (int mx : widths)
        for (int nx : grids)
            for (int per = 0; per < 2; ++per)
                for (int kind = 0; kind < 4; ++kind)
                    for (int rep = 0; rep < 3; ++rep) {
                        const Table t = make(mx, nx, per != 0, kind);
                        const int my = 1 + draw(3);
                        // the tile map against a running counter
                        long long w = 0;
                        for (int J = 0; J < my; ++J)
                            for (int I0 = 0; I0 < mx; I0 += kRegridTile, ++w) {
                                int32_t gJ = -1, gI0 = -1;
                                CHECK(regrid_tile(w, my, mx, &gJ, &gI0) && gJ == J && gI0 == I0);
                            }
                        int32_t dJ, dI;
                        CHECK(w == regrid_tiles_x(mx) * my && !regrid_tile(w, my, mx, &dJ, &dI) && !regrid_tile(-1, my, mx, &dJ, &dI));
                        int32_t widest = 0;
                        for (int I0 = 0; I0 < mx; I0 += kRegridTile) {
                            const int I1 = I0 + kRegridTile < mx ? I0 + kRegridTile : mx;
                            const RegridSpan sp = regrid_tile_span(t.first.data(), t.ptr.data(), mx, nx, t.periodic, I0);
                            widest = sp.width > widest ? sp.width : widest;
                            CHECK(sp.width >= 0 && sp.c0 >= 0 && sp.c0 < nx);
                            CHECK(t.periodic || sp.c0 + sp.width <= nx);
                            // the LDS row of the tile: exactly `width` slots, each the source column it stands for
                            std::vector<int32_t> held(static_cast<size_t>(sp.width), -1);
                            for (int s = 0; s < sp.width; ++s) {
                                const int32_t col = regrid_source_col(sp.c0, s, nx, t.periodic);
                                CHECK(col >= 0 && col < nx && col == (sp.c0 + s) % nx);
                                held.at(static_cast<size_t>(s)) = col;
                            }
                            const int rows = 1 + draw(3), r = draw(rows);
                            long long reach = 0;
                            bool any = false;
                            for (int I = I0; I < I1; ++I) {
                                const int cnt = t.ptr[I + 1] - t.ptr[I];
                                if (cnt == 0) continue;
                                any = true;
                                const int32_t off = regrid_lane_offset(t.first[I], sp.c0, nx, t.periodic);
                                CHECK(off >= 0 && off + cnt <= sp.width);
                                reach = off + cnt > reach ? off + cnt : reach;
                                for (int k = 0; k < cnt; ++k) {
                                    const int32_t slot = regrid_lds_slot(rows, sp.width, r, off, k);
                                    const bool fits = static_cast<long long>(r) * sp.width + off + k < kRegridLdsDwords;
                                    CHECK(fits ? slot == r * sp.width + off + k : slot == -1);
                                    // the sample the definition names for entry k of the run
                                    CHECK(held.at(static_cast<size_t>(off + k)) == (t.first[I] + k) % nx);
                                }
                                CHECK(regrid_lds_slot(rows, sp.width, r, off, cnt + sp.width) == -1);
                            }
                            CHECK(reach == sp.width);    // the smallest span that holds every run from its start
                            CHECK(any || (sp.c0 == 0 && sp.width == 0));
                            if (!t.periodic && any) {    // and it starts at the least first column
                                int least = nx;
                                for (int I = I0; I < I1; ++I)
                                    if (t.ptr[I + 1] > t.ptr[I] && t.first[I] < least) least = t.first[I];
                                CHECK(sp.c0 == least);
                            }
                        }
                        CHECK(regrid_max_width(t.first.data(), t.ptr.data(), mx, nx, t.periodic) == widest);
                        int longest = 0;
                        for (int I = 0; I < mx; ++I) longest = t.ptr[I + 1] - t.ptr[I] > longest ? t.ptr[I + 1] - t.ptr[I] : longest;
                        CHECK(regrid_max_run(t.ptr.data(), mx) == longest);
                        // the fit and the class, by their definition
                        for (int rows = 0; rows <= kRegridMaxRun; rows += 1 + draw(9)) {
                            const bool fit = rows >= 1 && widest >= 1 && static_cast<long long>(rows) * widest <= kRegridLdsDwords &&
                                             (t.periodic || widest <= nx);
                            CHECK(regrid_fits(rows, widest, nx, t.periodic) == fit);
                            const int lanes = mx < kRegridTile ? mx : kRegridTile;
                            const bool pick = static_cast<long long>(rows) * widest <= 4096 && widest >= 2 * lanes;
                            CHECK(regrid_auto_staged(rows, widest, lanes) == pick);
                            CHECK(regrid_class(rows, widest, lanes, nx, t.periodic, 1) == kRegridDirect);
                            CHECK(regrid_class(rows, widest, lanes, nx, t.periodic, 0) == (fit && pick ? kRegridStaged : kRegridDirect));
                            CHECK(regrid_class(rows, widest, lanes, nx, t.periodic, 2) == (fit ? kRegridStaged : kRegridDirect));
                            CHECK(regrid_class(rows, widest, lanes, nx, t.periodic, 3) == kRegridNone);
                        }
                    }
    // outside: no span, no offset, no column
    const int32_t f[2] = {0, 1}, p[3] = {0, 1, 2};
    CHECK(regrid_tile_span(f, p, 2, 4, false, 2).width == 0 && regrid_tile_span(nullptr, p, 2, 4, false, 0).width == 0);
    CHECK(regrid_lane_offset(1, 2, 4, false) == -1 && regrid_lane_offset(1, 2, 4, true) == 3 && regrid_lane_offset(4, 0, 4, true) == -1);
    CHECK(regrid_source_col(3, 1, 4, false) == -1 && regrid_source_col(3, 1, 4, true) == 0 && regrid_source_col(3, -1, 4, true) == -1);
}

static void check_layout() {
    for (int my = 0; my < 5; ++my)
        for (int mx = 0; mx < 600; mx += 1 + draw(120))
            for (int rep = 0; rep < 4; ++rep) {
                const long long n_ay = draw(300), n_ax = draw(40000);
                const RegridLayout l = regrid_layout(my, mx, n_ay, n_ax);
                const long long tx = (mx + 255) / 256;
                const long long sizes[10] = {my, my + 1, n_ay, my, mx, mx + 1, n_ax, mx, tx, tx};
                const int64_t at[10] = {l.row_first, l.row_ptr, l.ay, l.wy, l.col_first, l.col_ptr, l.ax, l.wx, l.tile_c0, l.tile_w};
                long long run = 0;
                for (int k = 0; k < 10; ++k) {
                    CHECK(at[k] == run);                 // the tables follow each other without a gap or an overlap
                    run += sizes[k];
                }
                CHECK(l.total == run);
            }
    CHECK(regrid_layout(-1, 2, 0, 0).total == 0);
}

static void check_chunks() {
    for (long long nt = 0; nt <= 70; ++nt)
        for (long long per = 0; per <= 75; ++per) {
            const long long nchunks = regrid_chunks(nt, per);
            CHECK(nchunks == (nt > 0 && per > 0 ? (nt + per - 1) / per : 0));
            long long next = 0;
            for (long long k = 0; k < nchunks; ++k) {
                int64_t t0, t1;
                regrid_chunk(k, nt, per, &t0, &t1);
                CHECK(t0 == next && t1 > t0 && t1 - t0 <= per && t1 <= nt);
                next = t1;
            }
            CHECK(next == (nchunks ? nt : 0));
            int64_t t0, t1;
            regrid_chunk(nchunks, nt, per, &t0, &t1);
            CHECK(t0 == 0 && t1 == 0);
            regrid_chunk(-1, nt, per, &t0, &t1);
            CHECK(t0 == 0 && t1 == 0);
        }
    // the automatic chunk: a multiple of 4 steps, one chunk at least, never more steps than about the cap allows
    for (long long nt : {1LL, 3LL, 23LL, 366LL, 14610LL})
        for (long long wg : {1LL, 6LL, 540LL, 4320LL, 100000LL})
            for (long long work : {0LL, 1LL, 4LL, 16LL, 100LL, 4096LL}) {
                const long long per = regrid_auto_chunk(nt, wg, work);
                const long long cap = 256 / (work > 0 ? work : 1) < 4 ? 4 : 256 / (work > 0 ? work : 1) > 64 ? 64 : 256 / (work > 0 ? work : 1);
                CHECK(per >= 1 && per % 4 == 0 && per <= (cap > nt ? (nt + 3) / 4 * 4 : cap + 3));
                CHECK(regrid_chunks(nt, per) >= 1);
            }
    CHECK(regrid_auto_chunk(0, 10, 10) == 1);
}

int main() {
    check_tiles_and_spans();
    check_layout();
    check_chunks();
    std::printf("%lld\n", checks);
    return 0;
}
