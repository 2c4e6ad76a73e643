// stable_desc.h -- the project's ONE stable descending order of fp32 values, for every source that ranks by score
// (topk.hip, grounding.hip): values descending, equal values by ascending index, -0.0 == +0.0, NaN in front of every number
// (NaNs equal among themselves) -- torch.sort(descending=True, stable=True).  An entry is key << 32 | (0xFFFFFFFF - index);
// its unsigned order is that order (larger = earlier), and 0 is below every entry.  Internal linkage (one copy per TU).
#ifndef ZIRA_STABLE_DESC_H_
#define ZIRA_STABLE_DESC_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Unsigned order == the sort's order.  Integer tests only: a comparison in a flushing float mode would tie denormals with zero.
__device__ __forceinline__ uint32_t key_of(float x)
{
    const uint32_t u = __float_as_uint(x);
    const uint32_t mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return 0xFFFFFFFFu;   // NaN: in front of +inf (0xFF800000), all NaNs equal
    if (mag == 0u) return 0x80000000u;           // -0.0 and +0.0 are one value
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long entry_of(uint32_t key, uint32_t index)
{
    return ((unsigned long long)key << 32) | (0xFFFFFFFFu - index);
}

__device__ __forceinline__ uint32_t index_of(unsigned long long entry)
{
    return 0xFFFFFFFFu - (uint32_t)entry;
}

// Bitonic network over P = 2^p entries (P <= blockDim.x), descending; thread t owns entry t and passes v = 0 for t >= P.
// The steps inside a wave are register exchanges, the steps across waves go through `exch` (P entries of LDS).  Every thread
// of the block calls it.  An exchange starts with a barrier, so what the caller read from `exch` before the call is safe.
__device__ __forceinline__ unsigned long long bitonic_desc(unsigned long long v, int P, unsigned long long *exch)
{
    const int t = threadIdx.x;
#pragma unroll 1
    for (int kk = 2; kk <= P; kk <<= 1) {
#pragma unroll 1
        for (int j = kk >> 1; j > 0; j >>= 1) {
            unsigned long long o;
            if (j >= 64) {
                __syncthreads();
                if (t < P) exch[t] = v;
                __syncthreads();
                o = t < P ? exch[t ^ j] : 0ull;
            } else {
                o = __shfl_xor(v, j);
            }
            const bool take_max = ((t & j) == 0) == ((t & kk) == 0);
            v = take_max ? (v > o ? v : o) : (v < o ? v : o);
        }
    }
    return v;
}

}  // namespace

#endif  // ZIRA_STABLE_DESC_H_
