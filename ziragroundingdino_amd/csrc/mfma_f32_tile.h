// mfma_f32_tile.h -- the 32 x 32 tile idiom of `v_mfma_f32_32x32x2_f32` (exact fp32 products, fp32 accumulation: the numerics of
// an fmaf chain), one definition for every source that builds on it.  Everything here is internal linkage (one copy per TU), so
// the kernels that use it keep their `(anonymous namespace)::` names.
//
// The operand ORIENTATION is chosen so that no tile is ever transposed or moved between lanes:
//   * a 32 x 32 result has its column on the lane (lane & 31) and 16 of its rows in the lane's registers:
//     row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -- rowmap(reg, lane >> 5).
//   * an instruction contracts over two k-indices, one from each lane half, and WHICH two is free as long as both operands agree.
//     So when the contraction runs over features, half h supplies feature 16 h + t at step t of a 16-step chain (32 h + t of a
//     32-step one): a lane loads a CONTIGUOUS half row (load_floats).  When it runs over the rows of a previous result, half h
//     supplies row rowmap(t, h): register t of the previous accumulator IS the operand, untouched, with no trip through LDS.
//   * hence S^T = K Q^T (keys x queries) puts a query's scores in ONE lane (two, with the other half: xhalf), softmax statistics
//     are per-lane scalars, and O^T += V^T P^T sums over S^T's rows (csrc/attn.hip, csrc/winattn.hip).
#ifndef ZIRA_MFMA_F32_TILE_H_
#define ZIRA_MFMA_F32_TILE_H_

#include <hip/hip_runtime.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the row of accumulator register reg in lane half hh (int or unsigned)
template <typename I>
__device__ __forceinline__ I rowmap(I reg, I hh) { return (reg & I(3)) + I(8) * (reg >> 2) + I(4) * hh; }

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.f;
    return z;
}

// N (16 or 32) consecutive floats from a 16-byte aligned address
template <int N>
__device__ __forceinline__ void load_floats(const float *p, float (&x)[N])
{
    static_assert(N == 16 || N == 32, "load_floats: half a row of 32 or of 64");
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        const float4 v = reinterpret_cast<const float4 *>(p)[i];
        x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
    }
}

// x of the same column's lane in the other half
__device__ __forceinline__ float xhalf(float x) { return __shfl_xor(x, 32); }

// acc += the N-step (16 or 32) chain of products of a[t] and b[t].  a and b: anything with operator[] -- register arrays, an
// f32x16 (a previous result as the operand), or a functor for an expression such as q[t] * scale
template <int N, typename A, typename B>
__device__ __forceinline__ void mfma_chain(const A &a, const B &b, f32x16 &acc)
{
#pragma unroll
    for (int t = 0; t < N; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
}

// rowmap's column-wise twin, for a tile kept TRANSPOSED (the lane's row r = lane & 31 of the matrix on the lane, 16 of the row's
// 32 columns in its registers): registers 4 q ... 4 q + 3 <-> the four consecutive columns col0 + 8 q + 4 hh ... of the lane's
// row, one 16-byte access each.  rowp: the lane's row, 16-byte aligned at col0
__device__ __forceinline__ void store_tile(float *rowp, int col0, int hh, const f32x16 &a)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4 *>(rowp + col0 + 8 * q + 4 * hh) = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
}

template <typename A>      // (an f32x16 or a register array)
__device__ __forceinline__ void load_tile(const float *rowp, int col0, int hh, A &a)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(rowp + col0 + 8 * q + 4 * hh);
        a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}

}  // namespace

#endif  // ZIRA_MFMA_F32_TILE_H_
