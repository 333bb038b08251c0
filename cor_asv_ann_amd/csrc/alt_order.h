// The total order of a row's entries that score_alternatives_kernel (train_kernels.hip) and sample_kernel (sample_kernels.hip)
// select by, and the wave-wide maximum their K selection rounds are made of.
#pragma once
#include "common.h"

namespace casv {

// The order is total: x descending as floats (the two zeros equal), the lower index first among equals.  One 64-bit key holds it:
// the float's bits made monotone (sign bit set for the positives, all bits flipped for the negatives; -0.0 taken as +0.0) above
// ~index, so a larger key is an earlier place.  No key of a valid row is 0 or all ones (those are NaN bit patterns).
__device__ __forceinline__ unsigned long long alt_key(float x, int v) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (0xffffffffu - (unsigned)v);
}
template <int MASK> __device__ __forceinline__ unsigned long long max_across(unsigned long long v) {
    const unsigned lo = (unsigned)lane_xor<MASK>((int)(unsigned)v), hi = (unsigned)lane_xor<MASK>((int)(unsigned)(v >> 32));
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > v ? o : v;
}
// the largest key of the wave, in every lane
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long top) {
    top = max_across<32>(top); top = max_across<16>(top); top = max_across<8>(top);
    top = max_across<4>(top); top = max_across<2>(top); top = max_across<1>(top);
    return top;
}

}  // namespace casv
