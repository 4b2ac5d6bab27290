// The integer rules of anomaly_distribution() (xmhw_amd/csrc/hist_bin.h) against plain integer arithmetic:
//   the bin       hist_bin_floor() against the floor of the integer division, for EVERY q in (-2^23, 2^23), for lo_q in
//                 {-2^23, -524288, 0, 3, 2^23 - 1} and width_q in {1, 2, 3, 8192, 8193, 65535, 65536, 1000003, 2^24}: the
//                 shift of a power of two and the reciprocal with its one correction step; and hist_row() on the result;
//   the halves    dword and addend of every b < 256: replayed into a column of 128 dwords, every bin once, then every
//                 dword holds 0x00010001, and a heap column of exactly hist_dwords(B) dwords takes every b < B;
//   the rank      hist_rank() for p_q in {0, 1, 2^31, 2^32 - 1, 2^32} and n in {0, 1, 2, 3, 65535, 2^31 - 1} against
//                 max(1, ceil(p_q * n / 2^32)) in 128-bit integers.
// Prints the number of cases compared.  Built with the host compiler under AddressSanitizer and UBSan by
// tests/test_host_hist_bin.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/hist_bin.h"

namespace {

long long g_checked = 0;

long long floor_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

void bins() {
    const int64_t los[] = {-(int64_t{1} << 23), -524288, 0, 3, (int64_t{1} << 23) - 1};
    const int32_t widths[] = {1, 2, 3, 8192, 8193, 65535, 65536, 1000003, 1 << 24};
    const int32_t B = 256;
    for (int64_t lo : los)
        for (int32_t w : widths) {
            const xmhw::HistBins h = xmhw::hist_bins(lo, w, B);
            const bool pow2 = (w & (w - 1)) == 0;
            if ((h.shift >= 0) != pow2 || (pow2 && (int32_t{1} << h.shift) != w)) {
                std::fprintf(stderr, "shift of width %d: %d\n", w, h.shift);
                std::exit(1);
            }
            for (int32_t q = -(1 << 23) + 1; q < (1 << 23); ++q) {
                const long long want = floor_div(static_cast<long long>(q) - lo, w);
                const int32_t got = xmhw::hist_bin_floor(h, q);
                const int32_t row = xmhw::hist_row(got, B);
                const int32_t want_row = want < 0 ? 0 : want >= B ? B + 1 : static_cast<int32_t>(1 + want);
                if (got != want || row != want_row) {
                    std::fprintf(stderr, "bin: lo=%lld w=%d q=%d: %d (row %d), expected %lld (row %d)\n",
                                 static_cast<long long>(lo), w, q, got, row, want, want_row);
                    std::exit(1);
                }
                ++g_checked;
            }
        }
}

void halves() {
    std::vector<uint32_t> column(128, 0u);
    for (int32_t b = 0; b < 256; ++b) {
        const int32_t dw = xmhw::hist_half_dword(b);
        const uint32_t add = xmhw::hist_half_addend(b);
        if (dw != b / 2 || add != (b % 2 ? 0x10000u : 1u)) {
            std::fprintf(stderr, "half: b=%d dword %d addend %u\n", b, dw, add);
            std::exit(1);
        }
        column.at(dw) += add;
        ++g_checked;
    }
    for (uint32_t v : column)
        if (v != 0x00010001u) {
            std::fprintf(stderr, "half: a dword holds %u\n", v);
            std::exit(1);
        }
    for (int32_t B = 1; B <= 256; ++B) {             // a column of exactly hist_dwords(B) dwords holds every bin of B
        uint32_t* col = new uint32_t[xmhw::hist_dwords(B)]();
        for (int32_t b = 0; b < B; ++b) col[xmhw::hist_half_dword(b)] += xmhw::hist_half_addend(b);
        delete[] col;
    }
}

void ranks() {
    const uint64_t ps[] = {0, 1, uint64_t{1} << 31, (uint64_t{1} << 32) - 1, uint64_t{1} << 32};
    const int32_t ns[] = {0, 1, 2, 3, 65535, 2147483647};
    for (uint64_t p : ps)
        for (int32_t n : ns) {
            const unsigned __int128 prod = static_cast<unsigned __int128>(p) * static_cast<unsigned __int128>(n);
            unsigned __int128 want = (prod + ((static_cast<unsigned __int128>(1) << 32) - 1)) >> 32;
            if (want < 1) want = 1;
            const int64_t got = xmhw::hist_rank(p, n);
            if (static_cast<unsigned __int128>(got) != want || got > (n > 1 ? n : 1)) {
                std::fprintf(stderr, "rank: p_q=%llu n=%d: %lld\n", static_cast<unsigned long long>(p), n,
                             static_cast<long long>(got));
                std::exit(1);
            }
            ++g_checked;
        }
}

}  // namespace

int main() {
    bins();
    halves();
    ranks();
    std::printf("%lld\n", g_checked);
    return 0;
}
