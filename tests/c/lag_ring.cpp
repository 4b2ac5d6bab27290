// The history arithmetic of lag_correlation() (xmhw_amd/csrc/lag_ring.h) against a brute-force lookup: a lane of the
// kernel is replayed on the host -- clear the ring, rebuild it from the warm-up range, then store, push and read the lags
// step by step -- and every (step, lag) it would read is compared with the series itself.  For every L from 0 to 63 in its
// own ring depth and in every deeper one, for series shorter and longer than L, for one block, for blocks that start at
// 0, 1, L - 1, L, L + 1, and for every block start of forced blocks of 1 and of 7 steps.  Prints the number of lookups
// compared.  Built with the host compiler under AddressSanitizer and UBSan by tests/test_host_lag_ring.py: the ring is a
// heap array of exactly `depth` slots, so a slot outside it is reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xmhw_amd/csrc/lag_ring.h"

namespace {

long long g_checked = 0;

[[noreturn]] void die(const char* what, int T, int L, int depth, int t0, int t, int l) {
    std::fprintf(stderr, "%s: T=%d L=%d depth=%d t0=%d t=%d l=%d\n", what, T, L, depth, t0, t, l);
    std::exit(1);
}

// qy of step s (0 where not valid) and its validity, by construction: every 5th and 7th step is not valid, and one run
// of 70 steps, longer than any lag
bool valid_at(int s) { return s % 5 != 3 && s % 7 != 6 && !(s >= 100 && s < 170); }
int32_t value_at(int s) { return valid_at(s) ? 1000 + 3 * s : 0; }

// the block [t0, t1) of a series of T steps, as the kernel walks it
void block(int T, int L, int depth, int t0, int t1) {
    std::vector<int32_t> ring(static_cast<size_t>(depth), 0);           // cleared: steps below 0 hold 0
    uint64_t mask = 0;
    const int32_t w0 = xmhw::lag_warmup_begin(t0, L);
    if (w0 != (t0 - L > 0 ? t0 - L : 0) || w0 < 0 || w0 > t0) die("warm-up range", T, L, depth, t0, w0, 0);
    for (int32_t t = w0; t < t0; ++t) {
        ring.at(static_cast<size_t>(xmhw::lag_ring_slot(t, 0, depth))) = value_at(t);
        mask = xmhw::lag_mask_push(mask, valid_at(t), L);
    }
    for (int32_t t = t0; t < t1; ++t) {
        ring.at(static_cast<size_t>(xmhw::lag_ring_slot(t, 0, depth))) = value_at(t);
        mask = xmhw::lag_mask_push(mask, valid_at(t), L);
        if (L < 63 && (mask >> (L + 1)) != 0) die("mask bits past L", T, L, depth, t0, t, L + 1);
        for (int l = 0; l <= L; ++l) {
            const int slot = xmhw::lag_ring_slot(t, l, depth);
            if (slot < 0 || slot >= depth) die("slot outside the ring", T, L, depth, t0, t, l);
            const int s = t - l;
            const bool want_valid = s >= 0 && valid_at(s);
            const int32_t want = s >= 0 ? value_at(s) : 0;
            if ((xmhw::lag_mask_bit(mask, l) != 0) != want_valid) die("mask bit", T, L, depth, t0, t, l);
            if (((xmhw::lag_mask_group(mask, l & ~15) >> (l & 15)) & 1u) != (want_valid ? 1u : 0u))
                die("mask bit of the lag group", T, L, depth, t0, t, l);
            if (ring.at(static_cast<size_t>(slot)) != want) die("ring value", T, L, depth, t0, t, l);
            ++g_checked;
        }
    }
}

void blocks_of(int T, int L, int depth, int bs) {
    for (int t0 = 0; t0 < T; t0 += bs) block(T, L, depth, t0, t0 + bs < T ? t0 + bs : T);
}

}  // namespace

int main() {
    const int depths[] = {16, 32, 64};
    for (int L = 0; L <= xmhw::kLagRingMaxLag; ++L) {
        const int own = xmhw::lag_ring_depth(L);
        if (own < L + 1 || (own != 16 && own / 2 >= L + 1)) die("ring depth", 0, L, own, 0, 0, 0);
        for (int depth : depths) {
            if (depth < own) continue;
            for (int T : {1, 2, L > 1 ? L - 1 : 1, L > 0 ? L : 1, L + 1, L + 2, 200, 257}) {
                blocks_of(T, L, depth, T);                               // one block
                blocks_of(T, L, depth, 1);                               // every block start of a forced block of 1
                blocks_of(T, L, depth, 7);                               // ... and of 7
                for (int t0 : {0, 1, L - 1, L, L + 1})                   // a block from t0 to the end
                    if (t0 >= 0 && t0 < T) block(T, L, depth, t0, T);
            }
        }
    }
    std::printf("%lld\n", g_checked);
    return 0;
}
