// count_above_desc() (xmhw_amd/csrc/sorted_count.h: the count of a descending run's keys above a value, put together from
// XORs of the nested compares) against the plain count: every descending run of N keys drawn from four distinct values and
// 0 (the "no key" value) -- every tie pattern --, N = 2 .. 9 (the sorted-list kernel uses 3 .. 9; 8 and 9 are the lists of
// the 37..48-track records), at the thresholds 0, every value, every value - 1 and + 1, and all ones.
// tests/test_host_sorted_count.py builds this with the host compiler and runs it.
#include <stdint.h>
#include <stdio.h>

#include "../../xmhw_amd/csrc/sorted_count.h"

// (either side of the sign bit: the compare is unsigned; the largest value + 1 is all ones)
static const uint32_t kValues[5] = {0xFFFFFFFEu, 0x80000001u, 0x7FFFFFFFu, 3u, 0u};

static long long g_cases = 0, g_wrong = 0;

template <int N>
static void check_run(const uint32_t (&u)[N]) {
    uint32_t th[2 + 3 * 4];
    int nt = 0;
    th[nt++] = 0u;
    th[nt++] = 0xFFFFFFFFu;
    for (int v = 0; v < 4; ++v) {
        th[nt++] = kValues[v];
        th[nt++] = kValues[v] - 1u;
        th[nt++] = kValues[v] + 1u;
    }
    for (int t = 0; t < nt; ++t) {
        uint32_t want = 0;
        for (int i = 0; i < N; ++i) want += u[i] > th[t] ? 1u : 0u;
        const uint32_t got = xmhw::count_above_desc<N>(u, th[t]);
        ++g_cases;
        if (got != want) {
            if (g_wrong < 10) {
                printf("N = %d, threshold %08x: got %u, the plain count is %u; run:", N, th[t], got, want);
                for (int i = 0; i < N; ++i) printf(" %08x", u[i]);
                printf("\n");
            }
            ++g_wrong;
        }
    }
}

// every non-increasing sequence over kValues: position i takes a value index not below position i - 1's
template <int N>
static void all_runs(uint32_t (&u)[N], int pos, int first) {
    if (pos == N) {
        check_run<N>(u);
        return;
    }
    for (int v = first; v < 5; ++v) {
        u[pos] = kValues[v];
        all_runs<N>(u, pos + 1, v);
    }
}

template <int N>
static void length() {
    uint32_t u[N];
    all_runs<N>(u, 0, 0);
}

int main() {
    length<2>();
    length<3>();
    length<4>();
    length<5>();
    length<6>();
    length<7>();
    length<8>();
    length<9>();
    printf("{\"cases\": %lld, \"wrong\": %lld}\n", g_cases, g_wrong);
    return g_wrong == 0 ? 0 : 1;
}
