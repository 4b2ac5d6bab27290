// sorted_count.h -- how many keys of a DESCENDING run lie above a value, without adding up one compare per key.
//
// The sorted-list kernel (kernels_sorted.hip, step 3) counts the keys of a row's new list above the carried boundary.  The run
// is sorted, so the compares M_p = [u[p - 1] > th], p = 1 .. N, are NESTED (M_1 >= M_2 >= ...) and the count c is a
// position: the multiples of 2^k among 1 .. c are floor(c / 2^k) many, so
//
//     bit k of c  =  XOR of M_p over the p that are multiples of 2^k.
//
// On the device a compare leaves its answer as a lane mask in a scalar register pair, the XORs are scalar instructions
// (N - 1 of them: the p with the same number of trailing zeros are folded first, bit k = that fold ^ bit k + 1), and the
// count is put together from its bits, highest first, by one add-with-carry per bit (c = c + c + bit): N compares and
// floor(log2 N) + 1 vector instructions where a plain count has N compares and N adds or selects.
//
// The rule is the same code for host and device; only the three primitives under it differ (a lane mask against a bool), so
// tests/c/sorted_count.cpp checks it with a host compiler against the plain count.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XMHW_HD __host__ __device__
#define XMHW_COUNT_UNROLL _Pragma("unroll")
#else
#define XMHW_HD
#define XMHW_COUNT_UNROLL
#endif

namespace xmhw {
namespace sorted_count {

#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned long long mask_t;      // a lane mask (the wave's answer to one vector compare)
__device__ __forceinline__ mask_t above(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 34); }     // 34: unsigned >
__device__ __forceinline__ uint32_t first_bit(mask_t m) { return __builtin_amdgcn_inverse_ballot_w64(m) ? 1u : 0u; }
// c + c + bit.  `m` must be the result of a SCALAR instruction (it is: an XOR of masks): a vector instruction may not read a
// scalar register a vector compare wrote two or fewer instructions earlier, and nobody counts wait states around an asm.
__device__ __forceinline__ uint32_t twice_plus(uint32_t c, mask_t m) {
    uint32_t r;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %1" : "=v"(r), "+s"(m) : "v"(c));
    return r;
}
#else
typedef bool mask_t;
inline mask_t above(uint32_t a, uint32_t b) { return a > b; }
inline uint32_t first_bit(mask_t m) { return m ? 1u : 0u; }
inline uint32_t twice_plus(uint32_t c, mask_t m) { return c + c + (m ? 1u : 0u); }
#endif

constexpr int bits_of(int n) { return n <= 1 ? 1 : 1 + bits_of(n / 2); }
constexpr int trailing_zeros(int p) { return (p & 1) ? 0 : 1 + trailing_zeros(p / 2); }

}  // namespace sorted_count

// #{i : u[i] > th} for u[0] >= u[1] >= ... >= u[N - 1]
template <int N>
XMHW_HD inline uint32_t count_above_desc(const uint32_t (&u)[N], uint32_t th) {
    using namespace sorted_count;
    static_assert(N >= 2, "a run");
    constexpr int NB = bits_of(N);
    mask_t fold[NB];      // fold[k] = XOR of M_p over the p with exactly k trailing zeros
XMHW_COUNT_UNROLL
    for (int p = 1; p <= N; ++p) {
        const mask_t mp = above(u[p - 1], th);
        const int k = trailing_zeros(p);
        if (p == (1 << k)) fold[k] = mp;
        else fold[k] = fold[k] ^ mp;
    }
    mask_t bit = fold[NB - 1];
    uint32_t c = first_bit(bit);
XMHW_COUNT_UNROLL
    for (int k = NB - 2; k >= 0; --k) {
        bit = fold[k] ^ bit;
        c = twice_plus(c, bit);
    }
    return c;
}

}  // namespace xmhw
