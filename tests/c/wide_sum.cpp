// The 128-bit sums of anomaly_distribution() (xmhw_amd/csrc/wide_sum.h) against __int128: a lane of the kernel is replayed
// on the host -- q^3 by wide_mac_i32(q^2, q), q^4 by wide_mac_u64(q^2, q^2) into a Wide in "registers", and a flush that
// adds the Wide to a (low, high) pair in "memory" by the carry rule of the header: old = low, low += v.lo (wrapping),
// high += wide_flush_high(v, old) -- and both the registers and the memory are compared with sums kept in __int128:
//   q = +-(2^23 - 1) alternating; all-positive and all-negative runs of 2^17 terms of the largest |q| (2^23);
//   random q; a low word that wraps upwards and downwards (a memory preset just below 2^64 and just above 0, and
//   addends of either sign); a flush after every term and after every 1,000, and one at the end.
// Prints the number of terms compared.  Built with the host compiler under AddressSanitizer and UBSan by
// tests/test_host_wide_sum.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/wide_sum.h"

namespace {

using i128 = __int128;
using u128 = unsigned __int128;

long long g_checked = 0;

[[noreturn]] void die(const char* what, const char* series, long long i) {
    std::fprintf(stderr, "%s: series %s, term %lld\n", what, series, i);
    std::exit(1);
}

bool equal(const xmhw::Wide& w, i128 v) {
    const u128 u = static_cast<u128>(v);
    return w.lo == static_cast<uint64_t>(u) && static_cast<uint64_t>(w.hi) == static_cast<uint64_t>(u >> 64);
}

struct Memory {                                      // a 128-bit accumulator in global memory and what it should hold
    uint64_t lo, hi;
    i128 want;
    Memory(uint64_t lo0, uint64_t hi0) : lo(lo0), hi(hi0), want(static_cast<i128>((static_cast<u128>(hi0) << 64) | lo0)) {}
    void flush(xmhw::Wide& v, i128& held) {
        if (v.lo != 0 || v.hi != 0) {                // as the kernel: nothing for a zero addend
            uint64_t high = static_cast<uint64_t>(v.hi);
            if (v.lo != 0) {
                const uint64_t old = lo;             // the atomic add that returns the old value
                lo += v.lo;
                high = xmhw::wide_flush_high(v, old);
            }
            hi += high;
        }
        want = static_cast<i128>(static_cast<u128>(want) + static_cast<u128>(held));
        v = xmhw::Wide{0, 0};
        held = 0;
    }
    bool holds() const { return lo == static_cast<uint64_t>(static_cast<u128>(want)) && hi == static_cast<uint64_t>(static_cast<u128>(want) >> 64); }
};

// the series through one lane: power 3 and power 4, a flush every `every` terms (0: at the end alone)
void replay(const std::vector<int32_t>& q, int every, uint64_t lo0, uint64_t hi0, const char* name) {
    xmhw::Wide v3{0, 0}, v4{0, 0};
    i128 h3 = 0, h4 = 0;
    Memory m3(lo0, hi0), m4(lo0, hi0);
    for (size_t i = 0; i < q.size(); ++i) {
        const int64_t q1 = q[i];
        const uint64_t q2 = static_cast<uint64_t>(q1 * q1);
        xmhw::wide_mac_i32(v3, q2, q[i]);
        xmhw::wide_mac_u64(v4, q2, q2);
        h3 += static_cast<i128>(q1) * q1 * q1;
        h4 += static_cast<i128>(q1) * q1 * q1 * q1;
        if (!equal(v3, h3)) die("q^3 in registers", name, static_cast<long long>(i));
        if (!equal(v4, h4)) die("q^4 in registers", name, static_cast<long long>(i));
        if (every > 0 && (i + 1) % every == 0) {
            m3.flush(v3, h3);
            m4.flush(v4, h4);
            if (!m3.holds()) die("q^3 in memory", name, static_cast<long long>(i));
            if (!m4.holds()) die("q^4 in memory", name, static_cast<long long>(i));
        }
        ++g_checked;
    }
    m3.flush(v3, h3);
    m4.flush(v4, h4);
    if (!m3.holds()) die("q^3 in memory at the end", name, -1);
    if (!m4.holds()) die("q^4 in memory at the end", name, -1);
}

}  // namespace

int main() {
    const int n = 1 << 17, top = (1 << 23) - 1, most = 1 << 23;
    std::vector<int32_t> alternating(n), positive(n, most), negative(n, -most), random(n), small(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) {
        alternating[i] = i % 2 ? -top : top;
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        random[i] = static_cast<int32_t>((s >> 33) % (2u * most + 1)) - most;
        small[i] = static_cast<int32_t>((s >> 40) % 7) - 3;            // zeros and tiny values: addends of a zero low or high word
    }
    struct Named {
        const std::vector<int32_t>* q;
        const char* name;
    };
    const Named all[] = {{&alternating, "alternating"}, {&positive, "positive"}, {&negative, "negative"}, {&random, "random"},
                         {&small, "small"}};
    // the memory presets: zero; a low word just below 2^64 (wraps upwards at the first positive flush); a low word just above
    // zero under a high word of -1 and of 0 (wraps downwards at the first negative flush)
    const uint64_t presets[][2] = {{0, 0}, {~0ull - 5, 7}, {3, ~0ull}, {3, 0}, {~0ull, ~0ull}};
    for (const Named& one : all)
        for (int every : {1, 1000, 0})
            for (const auto& p : presets) replay(*one.q, every, p[0], p[1], one.name);
    std::printf("%lld\n", g_checked);
    return 0;
}
