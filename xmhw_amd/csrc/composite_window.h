// composite_window.h -- the window of mhw_composite() (kernels_composite.hip): plain integer code without
// a device type, so that a host program can include it (tests/c/composite_window.cpp compares every function with a
// brute-force lookup of the bits).
//
// A lane of composite_accumulate walks the steps t of its cell upwards and carries a window of D = before + after + 1
// bits, D <= 64 * WORDS:
//     bit i of the window at step t is set  iff  the cell has an anchor at step t + before - i,   0 <= i < D,
// so the sample of step t lies at offset d = i - before from every anchor whose bit is set.  Steps below 0 and from Tn on
// hold no anchor.  The anchors come from the bitmap column of the cell, one bit per step, 64 steps a word; the code here
// takes it as load(w): word w of the column for 0 <= w < ceil(Tn / 64) with the bits at steps >= Tn zero, and 0 for every
// other w.
//   composite_window_at()   the window at step t0 from the bitmap words that cover [t0 - after, t0 + before]: WORDS + 1
//                           words, no sample -- what makes the blocks of a launch independent
//   CompositeWindow::push() t -> t + 1: shift left by one, insert the anchor bit of step t + 1 + before, mask to D bits
//   CompositeCursor         the look-ahead cursor that supplies that bit: it loads a word when the word changes
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XMHW_CW_HD __host__ __device__ __forceinline__
#else
#define XMHW_CW_HD inline
#endif
#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse64)
#define XMHW_CW_BITREVERSE64(x) __builtin_bitreverse64(x)
#endif
#endif

namespace xmhw {

// the lowest n bits; all of them from n = 64 on, none for n <= 0
XMHW_CW_HD uint64_t composite_low_bits(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1; }

// bit j <-> bit 63 - j
XMHW_CW_HD uint64_t composite_reverse(uint64_t x) {
#ifdef XMHW_CW_BITREVERSE64
    return XMHW_CW_BITREVERSE64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    return (x >> 32) | (x << 32);
#endif
}

template <int WORDS>
struct CompositeWindow {
    static_assert(WORDS == 1 || WORDS == 2, "one or two words");
    uint64_t w[WORDS];                               // w[0]: bits 0..63, w[1]: bits 64..127
    XMHW_CW_HD bool any() const { return (w[0] | w[WORDS - 1]) != 0; }
    // t -> t + 1: `bit` is the anchor bit of step t + 1 + before
    XMHW_CW_HD void push(uint32_t bit, int D) {
        if (WORDS == 2) w[WORDS - 1] = ((w[WORDS - 1] << 1) | (w[0] >> 63)) & composite_low_bits(D - 64);
        w[0] = ((w[0] << 1) | (bit & 1u)) & composite_low_bits(D);
    }
};

// The window at step t0.  Bit i is step t0 + before - i: the 64 * WORDS steps that end at t0 + before, taken from the
// WORDS + 1 bitmap words that hold them, reversed and cut to D bits.
template <int WORDS, typename Load>
XMHW_CW_HD CompositeWindow<WORDS> composite_window_at(Load&& load, int32_t t0, int32_t before, int D) {
    const int32_t s0 = t0 + before - (64 * WORDS - 1);   // the lowest of those steps, of either sign
    const int32_t w0 = s0 >> 6, r = s0 & 63;             // arithmetic shift: the floor for a negative s0 as well
    uint64_t x[WORDS + 1];
    for (int j = 0; j <= WORDS; ++j) x[j] = load(w0 + j);
    CompositeWindow<WORDS> win;
    for (int j = 0; j < WORDS; ++j) {
        const uint64_t steps = r ? (x[j] >> r) | (x[j + 1] << (64 - r)) : x[j];     // bit b = step s0 + 64 j + b
        win.w[WORDS - 1 - j] = composite_reverse(steps) & composite_low_bits(D - 64 * (WORDS - 1 - j));
    }
    return win;
}

// the anchor bit of step s >= 0 for an s that goes up from call to call: the word is loaded when it changes
struct CompositeCursor {
    int32_t wi = -1;
    uint64_t word = 0;
    template <typename Load>
    XMHW_CW_HD uint32_t bit(Load&& load, int32_t s) {
        if ((s >> 6) != wi) {
            wi = s >> 6;
            word = load(wi);
        }
        return static_cast<uint32_t>(word >> (s & 63)) & 1u;
    }
};

}  // namespace xmhw
