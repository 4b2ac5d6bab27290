// wide_sum.h -- the 128-bit sums of anomaly_distribution() (kernels_distribution.hip): the third and fourth
// powers of a fixed-point sample (|q| <= 2^23: |q^3| <= 2^69, q^4 <= 2^92) do not fit 64 bits, so their sums are 128-bit
// two's-complement integers kept as (low word uint64, high word int64).  Plain integer code without a device type, so
// that a host program can include it (tests/c/wide_sum.cpp compares every function with __int128).
//
//   a lane        adds products into a Wide in registers: 32 x 32 -> 64-bit partial products (v_mad_u64_u32 on the device)
//                 and a carry chain; a negative product is added as its two's complement.
//   a flush       adds the lane's Wide to the Wide in global memory under concurrent flushes of other workgroups: the low
//                 word by an atomic add that RETURNS the old value, the carry out of that addition derived from it
//                 (wide_carry) and added to the high word together with the lane's high word, by an atomic add without a
//                 return value.  Every atomic addition to the low word wraps at most once and reports it to exactly one
//                 flush, so the high word has received floor(sum of the low addends / 2^64) carries when all flushes are
//                 done: the pair is the exact sum modulo 2^128, in any order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XMHW_WS_HD __host__ __device__ __forceinline__
#else
#define XMHW_WS_HD inline
#endif

namespace xmhw {

struct Wide {
    uint64_t lo;
    int64_t hi;
};

// acc += (lo, hi), two's complement
XMHW_WS_HD void wide_add(Wide& acc, uint64_t lo, uint64_t hi) {
    const uint64_t s = acc.lo + lo;
    acc.hi = static_cast<int64_t>(static_cast<uint64_t>(acc.hi) + hi + (s < lo ? 1u : 0u));
    acc.lo = s;
}

// acc += a * s: a unsigned 64-bit, s signed 32-bit
XMHW_WS_HD void wide_mac_i32(Wide& acc, uint64_t a, int32_t s) {
    const uint32_t m = s < 0 ? 0u - static_cast<uint32_t>(s) : static_cast<uint32_t>(s);
    const uint64_t p0 = static_cast<uint64_t>(static_cast<uint32_t>(a)) * m;             // weight 1
    const uint64_t p1 = (a >> 32) * m;                                                  // weight 2^32, below 2^64
    uint64_t lo = p0 + (p1 << 32);
    uint64_t hi = (p1 >> 32) + (lo < p0 ? 1u : 0u);
    if (s < 0) {                                     // the two's complement of (lo, hi)
        lo = 0u - lo;
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
    wide_add(acc, lo, hi);
}

// acc += a * b: both unsigned 64-bit
XMHW_WS_HD void wide_mac_u64(Wide& acc, uint64_t a, uint64_t b) {
    const uint64_t a0 = static_cast<uint32_t>(a), a1 = a >> 32, b0 = static_cast<uint32_t>(b), b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    // the middle column: the high half of p00 and the low halves of p01 and p10 (below 3 * 2^32)
    const uint64_t mid = (p00 >> 32) + static_cast<uint32_t>(p01) + static_cast<uint32_t>(p10);
    const uint64_t lo = (mid << 32) | static_cast<uint32_t>(p00);
    const uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    wide_add(acc, lo, hi);
}

// the carry out of the atomic addition old_lo + add_lo that a flush made to the low word in memory
XMHW_WS_HD uint64_t wide_carry(uint64_t old_lo, uint64_t add_lo) { return old_lo + add_lo < old_lo ? 1u : 0u; }

// what a flush adds to the high word in memory: the lane's high word and that carry
XMHW_WS_HD uint64_t wide_flush_high(const Wide& v, uint64_t old_lo) {
    return static_cast<uint64_t>(v.hi) + wide_carry(old_lo, v.lo);
}

}  // namespace xmhw
