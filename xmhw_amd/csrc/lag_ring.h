// lag_ring.h -- the history of lag_correlation() (kernels_lagcorr.hip): plain integer code without a
// device type, so that a host program can include it (tests/c/lag_ring.cpp compares every function with a brute-force
// lookup).
//
// A lane of lag_corr_accumulate walks the steps t of its cell upwards.  For the lags l in [0, L], L <= 63, it needs the
// fixed-point value qy(t - l) of the second series and whether that step was valid:
//   the ring   `depth` slots per lane (a power of two, lag_ring_depth(L) >= L + 1), step s in slot s mod depth.  A step
//              that is not valid, and a step below 0, holds 0.  The lane stores step t before it reads the lags of step t,
//              so the slot of lag l holds step t - l while l < depth: the step stored there before it, t - l - depth, is
//              older than any lag.
//   the mask   bit l set iff step t - l exists and was valid, 0 <= l <= L.  t -> t + 1: shift left by one, insert the
//              validity of step t + 1, cut to L + 1 bits.
//   a block    that starts at t0 > 0 rebuilds both from the steps lag_warmup_begin(t0, L) .. t0 - 1, after clearing its
//              ring: it stores them and pushes their validity, and reduces and counts nothing from them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XMHW_LR_HD __host__ __device__ __forceinline__
#else
#define XMHW_LR_HD inline
#endif

namespace xmhw {

constexpr int kLagRingMaxLag = 63;

// the ring depth of a lag range [0, L]: 16, 32 or 64 slots, the least of them that holds L + 1 steps (8 slots would gain
// nothing: up to 32 slots the registers bound the occupancy, not the LDS)
XMHW_LR_HD int lag_ring_depth(int L) { return L < 16 ? 16 : L < 32 ? 32 : 64; }

// the slot of step t at lag l (step t - l, of either sign) in a ring of `depth` slots, a power of two
XMHW_LR_HD int lag_ring_slot(int32_t t, int l, int depth) {
    return static_cast<int>((static_cast<uint32_t>(t) - static_cast<uint32_t>(l)) & static_cast<uint32_t>(depth - 1));
}

// the first step a block that starts at t0 reads to rebuild its history: [lag_warmup_begin(t0, L), t0)
XMHW_LR_HD int32_t lag_warmup_begin(int32_t t0, int L) { return t0 > L ? t0 - L : 0; }

// the bits 0 .. L
XMHW_LR_HD uint64_t lag_mask_bits(int L) { return L >= 63 ? ~0ull : (1ull << (L + 1)) - 1; }

// t -> t + 1: `valid` is the validity of step t + 1
XMHW_LR_HD uint64_t lag_mask_push(uint64_t mask, bool valid, int L) {
    return ((mask << 1) | (valid ? 1ull : 0ull)) & lag_mask_bits(L);
}

// the bits of the lags l0, l0 + 1, ... as bits 0, 1, ... (l0 <= 63)
XMHW_LR_HD uint32_t lag_mask_group(uint64_t mask, int l0) { return static_cast<uint32_t>(mask >> l0); }

// is the partner of lag l valid
XMHW_LR_HD uint32_t lag_mask_bit(uint64_t mask, int l) { return static_cast<uint32_t>(mask >> l) & 1u; }

}  // namespace xmhw
