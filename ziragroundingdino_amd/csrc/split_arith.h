// split_arith.h -- the split arithmetic of the fp32-accurate matrix-core products ("GEMM arithmetic"), one definition
// for every source that uses it.  A group of fp32 numbers (a row, or a row's 32-deep K step) is scaled by the power of two that
// brings its largest magnitude into [2^14, 2^15); each scaled number is then a sum of planes: its round-to-nearest-even high plane
// and the exact remainders below it.
//   f16x2  (gemm_f16x2, gemm_f16x2_panel, thin_f16x2, ffn_f16x2): two f16 planes, a = a1 + a2 + rest, |rest| <= 2^-22 |a|.
//   bf16x3 (gemm_bf16x3, xty_bf16x3): three bfloat16 planes, no scale needed.
// Everything here is internal linkage (one copy per TU), so the kernels that use it keep their `(anonymous namespace)::` names.
#ifndef ZIRA_SPLIT_ARITH_H_
#define ZIRA_SPLIT_ARITH_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "mfma_f32_tile.h"   // f32x16

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- f16, two planes ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned pk_f16(float a, float b)
{
    f32x2 x = {a, b};
    f16x2 h = __builtin_convertvector(x, f16x2);   // round to nearest even
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float f16_lo(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[0]; }
__device__ __forceinline__ float f16_hi(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[1]; }

// the power of two that brings amax into [2^14, 2^15), and its reciprocal (exact); amax = 0 or tiny: 2^100; inf / NaN pass through
__device__ __forceinline__ void pow2_scale(float amax, float &s, float &inv)
{
    int e = (int)((__float_as_uint(amax) >> 23) & 0xFFu);   // amax in [2^(e-127), 2^(e-126))
    int se = 127 + 14 - (e - 127);                          // biased exponent of the scale
    se = se > 227 ? 227 : (se < 1 ? 1 : se);                // <= 2^100: the reciprocal stays a normal number
    s = __uint_as_float((unsigned)se << 23);
    inv = __uint_as_float((unsigned)(254 - se) << 23);
}

// pow2_scale with its two clamps applied in sequence: the same values, other instructions.  csrc/ffn_f16x2.hip uses this
// spelling, whose code its kernels were tuned with; a change to the scale is made to both.
__device__ __forceinline__ void pow2_scale_seq(float amax, float &s, float &inv)
{
    int e = (int)((__float_as_uint(amax) >> 23) & 0xFFu);
    int se = 127 + 14 - (e - 127);
    se = se > 227 ? 227 : se;
    se = se < 1 ? 1 : se;
    s = __uint_as_float((unsigned)se << 23);
    inv = __uint_as_float((unsigned)(254 - se) << 23);
}

// one fp32 number (already scaled) -> its two f16 planes: the low 16 bits of .x and .y
__device__ __forceinline__ uint2 split1_f16x2(float v)
{
    const unsigned p1 = pk_f16(v, 0.f);
    return make_uint2(p1, pk_f16(v - f16_lo(p1), 0.f));   // (exact difference)
}

// two fp32 numbers (already scaled) -> one packed pair of each plane
__device__ __forceinline__ void split2_f16x2(float x, float y, unsigned &p1, unsigned &p2)
{
    p1 = pk_f16(x, y);
    p2 = pk_f16(x - f16_lo(p1), y - f16_hi(p1));   // (exact differences)
}

// four fp32 numbers (already scaled) -> their two f16 planes, four halves (8 bytes) each
__device__ __forceinline__ void split4_f16x2(const float4 v, uint2 &p1, uint2 &p2)
{
    p1.x = pk_f16(v.x, v.y);
    p1.y = pk_f16(v.z, v.w);
    p2.x = pk_f16(v.x - f16_lo(p1.x), v.y - f16_hi(p1.x));   // (exact differences)
    p2.y = pk_f16(v.z - f16_lo(p1.y), v.w - f16_hi(p1.y));
}

// The largest of the 256 threads' partial maxima x, returned to every thread; red = 256 floats of LDS.  Ends with a barrier.
__device__ __forceinline__ float block_amax256(float x, float *red)
{
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

// Split weight fragments [N / 32][KS][2 planes][64 lanes][8 halves]: the offset in halves of plane 1's element (n, k) =
// (32 t + lm, k), with KS 16-deep matrix-core steps per column tile; plane 2's element is 512 halves further on.
__device__ __forceinline__ size_t frag_offset(int t, int lm, int k, int KS)
{
    const int st = k >> 4, hf = (k >> 3) & 1, e = k & 7;
    return (((size_t)t * KS + st) * 2) * 512 + (size_t)(hf * 32 + lm) * 8 + e;
}

// ---- bfloat16, three planes ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned pk_bf16(float a, float b)
{
    f32x2 x = {a, b};
    bf16x2 h = __builtin_convertvector(x, bf16x2);   // v_cvt_pk_bf16_f32: round to nearest even
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float bf_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(unsigned p) { return __uint_as_float(p & 0xFFFF0000u); }

// four fp32 numbers -> their three bfloat16 planes, four bfloat16 (8 bytes) each
__device__ __forceinline__ void split4_bf16x3(const float4 v, uint2 &p1, uint2 &p2, uint2 &p3)
{
    p1.x = pk_bf16(v.x, v.y);
    p1.y = pk_bf16(v.z, v.w);
    const float rx = v.x - bf_lo(p1.x), ry = v.y - bf_hi(p1.x), rz = v.z - bf_lo(p1.y), rw = v.w - bf_hi(p1.y);   // exact
    p2.x = pk_bf16(rx, ry);
    p2.y = pk_bf16(rz, rw);
    p3.x = pk_bf16(rx - bf_lo(p2.x), ry - bf_hi(p2.x));   // (the differences are exact, and fit bfloat16 exactly)
    p3.y = pk_bf16(rz - bf_lo(p2.y), rw - bf_hi(p2.y));
}

}  // namespace

#endif  // ZIRA_SPLIT_ARITH_H_
