// lane_sum.h -- sums across the lanes of a wave with DPP and permlane swaps (no LDS, no barriers), one definition for every
// source that uses them.  Everything here is internal linkage (one copy per TU).
#ifndef ZIRA_LANE_SUM_H_
#define ZIRA_LANE_SUM_H_

#include <hip/hip_runtime.h>

namespace {

// x + x of the lane that the DPP control CTRL names
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x)
{
    return x + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), CTRL, 0xf, 0xf, false));
}

// sum over the N (4, 8, 16, 32 or 64) consecutive lanes of an aligned group; every lane ends with its group's total
template <int N>
__device__ __forceinline__ float lane_sum(float x)
{
    static_assert(N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "lane_sum: N is 4, 8, 16, 32 or 64");
    x = dpp_add<0xB1>(x);                 // quad_perm:[1,0,3,2]   (xor 1)
    x = dpp_add<0x4E>(x);                 // quad_perm:[2,3,0,1]   (xor 2)
    if (N >= 8) x = dpp_add<0x141>(x);    // row_half_mirror       (xor 4 on quad sums)
    if (N >= 16) x = dpp_add<0x140>(x);   // row_mirror            (xor 8 on octet sums)
    if (N >= 32) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    }
    if (N == 64) {
        const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        x = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    }
    return x;
}

// the same for a double: its two halves travel through the same exchanges
__device__ __forceinline__ double halves_to_double(unsigned lo, unsigned hi)
{
    return __hiloint2double((int)hi, (int)lo);
}

template <int CTRL>
__device__ __forceinline__ double dpp_add(double x)
{
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2loint(x), CTRL, 0xf, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2hiint(x), CTRL, 0xf, 0xf, false);
    return x + halves_to_double(lo, hi);
}

template <int N>
__device__ __forceinline__ double lane_sum(double x)
{
    static_assert(N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "lane_sum: N is 4, 8, 16, 32 or 64");
    x = dpp_add<0xB1>(x);
    x = dpp_add<0x4E>(x);
    if (N >= 8) x = dpp_add<0x141>(x);
    if (N >= 16) x = dpp_add<0x140>(x);
    if (N >= 32) {
        const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        x = halves_to_double(a[0], b[0]) + halves_to_double(a[1], b[1]);
    }
    if (N == 64) {
        const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        x = halves_to_double(a[0], b[0]) + halves_to_double(a[1], b[1]);
    }
    return x;
}

// The wave's 64 doubles by the plain `__shfl_xor` butterfly, offsets 32 ... 1.  It stands beside lane_sum<64> because it adds
// in ANOTHER order (far partners first, neighbours last), and the order of the additions is part of the bits that the tests
// of its users pin: the side-branch nodes' loss and gradient sums were written with it and keep it.
__device__ __forceinline__ double lane_sum_xor64(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace

#endif  // ZIRA_LANE_SUM_H_
