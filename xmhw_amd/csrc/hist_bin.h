// hist_bin.h -- the integer rules of anomaly_distribution() (kernels_distribution.hip): plain integer code
// without a device type, so that a host program can include it (tests/c/hist_bin.cpp compares every function with plain
// integer division).
//
//   the bin      of a fixed-point sample q under bins (lo_q, width_q, B): b = floor((q - lo_q) / width_q), exactly.  b < 0
//                is the UNDER row (row 0 of a histogram), b >= B the OVER row (row B + 1), anything else row 1 + b.
//                |q| <= 2^23 and |lo_q| <= 2^23, so u = q - lo_q fits 26 bits.  A width that is a power of two is an
//                arithmetic shift; any other width is a float64 multiply by the reciprocal, floor, and ONE correction step
//                against b * width_q <= u < (b + 1) * width_q: the product u * (1 / w) is off by less than 2^-26 of a
//                bin, so its floor is off by one at most.
//   the halves   a lane counts in 16-bit halves of its own column of dwords: bin b is half b & 1 of dword b >> 1.
//   the rank     of a probability p_q = rint(p * 2^32) in [0, 2^32] among n samples: r = max(1, ceil(p_q * n / 2^32)), in
//                64-bit integers (p_q * n <= 2^63).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XMHW_HB_HD __host__ __device__ __forceinline__
#else
#define XMHW_HB_HD inline
#endif

namespace xmhw {

constexpr int32_t kHistMaxBins = 256;
constexpr int32_t kHistHalfMax = 65535;              // what a 16-bit half holds: a run is flushed after so many steps
constexpr int32_t kHistMaxEdge = 1 << 23;            // |lo_q| at most

struct HistBins {
    int32_t lo_q, width_q, B;
    int32_t shift;                                   // log2(width_q) where that is a whole number, else -1
    double recip;                                    // 1.0 / width_q
};

inline HistBins hist_bins(int64_t lo_q, int32_t width_q, int32_t B) {
    HistBins h{static_cast<int32_t>(lo_q), width_q, B, -1, 1.0 / static_cast<double>(width_q)};
    for (int s = 0; s < 31; ++s)
        if (width_q == (int32_t{1} << s)) h.shift = s;
    return h;
}

// floor((q - lo_q) / width_q) for |q| <= 2^23
XMHW_HB_HD int32_t hist_bin_floor(const HistBins& h, int32_t q) {
    const int32_t u = q - h.lo_q;
    if (h.shift >= 0) return u >> h.shift;           // (arithmetic: the floor for either sign)
    const double f = static_cast<double>(u) * h.recip;
    int32_t b = static_cast<int32_t>(f) - (f < 0.0 ? 1 : 0);           // at or one below the floor of f, within one of b
    const int32_t r = u - b * h.width_q;             // |b * width_q| <= |u| + 2 width_q < 2^27
    if (r < 0) --b;
    else if (r >= h.width_q) ++b;
    return b;
}

// the row of a histogram [0 .. B + 1] that bin index b counts in
XMHW_HB_HD int32_t hist_row(int32_t b, int32_t B) { return b < 0 ? 0 : b >= B ? B + 1 : 1 + b; }

// the packed halves: the dword of bin b in a lane's column and what one sample adds to it (0 <= b < B)
XMHW_HB_HD int32_t hist_half_dword(int32_t b) { return b >> 1; }
XMHW_HB_HD uint32_t hist_half_addend(int32_t b) { return 1u << (16 * (b & 1)); }
// the dwords of a column of B bins
XMHW_HB_HD int32_t hist_dwords(int32_t B) { return (B + 1) >> 1; }

// the rank of p_q among n >= 0 samples (1-based; 1 for n == 0 as well: the caller has no sample to give it)
XMHW_HB_HD int64_t hist_rank(uint64_t p_q, int32_t n) {
    const uint64_t r = (p_q * static_cast<uint64_t>(n) + 0xFFFFFFFFull) >> 32;
    return r < 1 ? 1 : static_cast<int64_t>(r);
}

}  // namespace xmhw
