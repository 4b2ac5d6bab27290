// The window of mhw_composite() (xmhw_amd/csrc/composite_window.h) against a brute-force lookup of the bits, on the host:
// for one and two words, every D from 1 to 128 (four splits into before and after each), every block start of a 200-step
// column (and of shorter ones), random and adversarial bitmaps.  The kernel compiles the same text.  Built with
// -fsanitize=address,undefined and run as a program (tests/test_host_composite_window.py); prints the number of window
// bits compared and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../xmhw_amd/csrc/composite_window.h"

namespace {

constexpr int kSteps = 200;                          // 3 words and 8 steps of a fourth

struct Column {
    std::vector<uint64_t> words;
    int T;
    explicit Column(int Tn) : words((Tn + 63) / 64, 0), T(Tn) {}
    void set(int t) { words[t >> 6] |= 1ull << (t & 63); }
    bool anchor(int t) const { return t >= 0 && t < T && ((words[t >> 6] >> (t & 63)) & 1); }
    // what the kernel's loader gives: 0 outside the column
    uint64_t load(int32_t w) const { return w >= 0 && w < static_cast<int32_t>(words.size()) ? words[w] : 0; }
};

uint64_t next_random(uint64_t& state) {              // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

std::vector<Column> columns() {
    std::vector<Column> out;
    for (int T : {kSteps, 1, 63, 64, 65, 128, 129}) {
        Column empty(T), full(T), edges(T), pairs(T), sparse(T), dense(T);
        for (int t = 0; t < T; ++t) full.set(t);
        for (int t : {0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, T - 2, T - 1})
            if (t >= 0 && t < T) edges.set(t);
        for (int t = 0; t < T; t += 37) {
            pairs.set(t);
            if (t + 1 < T) pairs.set(t + 1);
        }
        uint64_t state = 1234567 + T;
        for (int t = 0; t < T; ++t) {
            const uint64_t r = next_random(state);
            if (r % 29 == 0) sparse.set(t);
            if ((r >> 32) % 2 == 0) dense.set(t);
        }
        for (const Column& c : {empty, full, edges, pairs, sparse, dense}) out.push_back(c);
    }
    return out;
}

// the window of step t, bit by bit from the column
template <int WORDS>
xmhw::CompositeWindow<WORDS> brute(const Column& col, int before, int D, int t) {
    xmhw::CompositeWindow<WORDS> win;
    for (int h = 0; h < WORDS; ++h) win.w[h] = 0;
    for (int i = 0; i < D; ++i)
        if (col.anchor(t + before - i)) win.w[i >> 6] |= 1ull << (i & 63);
    return win;
}

template <int WORDS>
bool same(const xmhw::CompositeWindow<WORDS>& got, const xmhw::CompositeWindow<WORDS>& want, const char* what, int T, int before,
          int D, int t) {
    bool ok = got.any() == ((want.w[0] | want.w[WORDS - 1]) != 0);
    for (int h = 0; h < WORDS; ++h) ok = ok && got.w[h] == want.w[h];
    if (!ok)
        std::printf("%s: WORDS %d T %d before %d D %d t %d: got %016llx %016llx, expected %016llx %016llx\n", what, WORDS, T,
                    before, D, t, static_cast<unsigned long long>(got.w[WORDS - 1]), static_cast<unsigned long long>(got.w[0]),
                    static_cast<unsigned long long>(want.w[WORDS - 1]), static_cast<unsigned long long>(want.w[0]));
    return ok;
}

// Every block start t0 of the column: the warm-up gives the window of t0, and one push from it (a fresh cursor, as a block
// has) the window of t0 + 1 -- by induction every rolled window of every block.  Then one roll over the whole column with
// one cursor, which crosses every word edge.  Returns the window bits compared, -1 after a mismatch.
template <int WORDS>
long long check(const Column& col, int before, int D) {
    const auto load = [&](int32_t w) { return col.load(w); };
    xmhw::CompositeWindow<WORDS> rolled = xmhw::composite_window_at<WORDS>(load, 0, before, D);
    xmhw::CompositeCursor ahead;
    long long compared = 0;
    for (int t0 = 0; t0 < col.T; ++t0) {
        const xmhw::CompositeWindow<WORDS> want = brute<WORDS>(col, before, D, t0);
        xmhw::CompositeWindow<WORDS> win = xmhw::composite_window_at<WORDS>(load, t0, before, D);
        if (!same(win, want, "warm-up", col.T, before, D, t0)) return -1;
        xmhw::CompositeCursor fresh;
        win.push(fresh.bit(load, t0 + 1 + before), D);
        if (!same(win, brute<WORDS>(col, before, D, t0 + 1), "one push", col.T, before, D, t0 + 1)) return -1;
        if (t0 > 0) rolled.push(ahead.bit(load, t0 + before), D);
        if (!same(rolled, want, "rolled", col.T, before, D, t0)) return -1;
        compared += 3 * 64 * WORDS;
    }
    return compared;
}

}  // namespace

int main() {
    if (xmhw::composite_low_bits(0) != 0 || xmhw::composite_low_bits(-5) != 0 || xmhw::composite_low_bits(1) != 1 ||
        xmhw::composite_low_bits(63) != 0x7FFFFFFFFFFFFFFFull || xmhw::composite_low_bits(64) != ~0ull ||
        xmhw::composite_low_bits(70) != ~0ull) {
        std::printf("composite_low_bits\n");
        return 1;
    }
    for (int j = 0; j < 64; ++j)
        if (xmhw::composite_reverse(1ull << j) != 1ull << (63 - j) || xmhw::composite_reverse(~(1ull << j)) != ~(1ull << (63 - j))) {
            std::printf("composite_reverse bit %d\n", j);
            return 1;
        }
    long long compared = 0;
    const std::vector<Column> cols = columns();
    for (int D = 1; D <= 128; ++D) {
        // the splits of D: all of it after, all of it before, the middle, and an uneven one
        for (int before : {0, D - 1, (D - 1) / 2, (D - 1) / 3}) {
            for (const Column& col : cols) {
                const long long one = D <= 64 ? check<1>(col, before, D) : 0;
                const long long two = check<2>(col, before, D);
                if (one < 0 || two < 0) return 1;
                compared += one + two;
            }
        }
    }
    std::printf("%lld\n", compared);
    return 0;
}
