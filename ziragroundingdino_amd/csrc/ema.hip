// ema.hip -- the model exponential moving average on the device: update, swap and copy, ONE launch each over every fp32
// tensor of the model (C ABI: zira_ema_update_f32, zira_ema_swap_f32, zira_ema_copy_f32; contract in include/zira_msda.h).
//
// The averaged state is one flat fp32 buffer; the model's tensors stay where they are and are reached through the design of
// optim_tail.hip: a device table of segments (pointer, start in the flat buffer, numel) and block_segment[], the first segment
// of every block of kChunk flat elements.  Differences from that file:
//   * the grid is capped (kMaxGrid workgroups stride over the blocks): the state is the whole model, 170 M elements and
//     41 k blocks for Swin-T, and a streaming kernel gains nothing from more workgroups than the chip holds;
//   * segments may leave gaps (the Python side starts each on a multiple of 4 elements, so that a tensor from the allocator
//     and its twin share their phase modulo 16 bytes);
//   * a 16-byte access is a naturally aligned one, taken only where BOTH addresses of a run are 16-byte aligned; a run whose
//     two addresses differ in phase (a view at an odd offset) and the ends of every run go one dword per lane, coalesced.
// Memory-bound: update reads 8 and writes 4 bytes per element, swap 8 and 8, copy 4 and 4.  No LDS, no atomics, no
// workspace.  The arithmetic is spelled with explicit rounding intrinsics: the bits must be torch's _foreach_mul_ /
// _foreach_add_(alpha=) chain's, and whether that chain's second kernel holds an FMA is a property of the library's build that
// the caller states (`contracted`).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = ZIRA_EMA_CHUNK;
constexpr long long kMaxN = ZIRA_EMA_MAX_N;
constexpr long long kMaxGrid = 2048;   // 256 CUs x 8 workgroups: what the chip holds of a kernel this light
static_assert(kChunk % (4 * kThreads) == 0, "a block is a whole number of 16-byte rounds of the workgroup");

typedef float f4 __attribute__((ext_vector_type(4)));   // 16 bytes, 16-byte aligned

// torch._foreach_mul_(ema, decay); torch._foreach_add_(ema, p, alpha=alpha) -- the second as a multiply and an add
struct UpdateMulAdd {
    static constexpr bool kReadE = true, kReadP = true, kWriteE = true, kWriteP = false;
    float decay, alpha;
    __device__ __forceinline__ void operator()(float &e, float &p) const
    {
        e = __fadd_rn(__fmul_rn(e, decay), __fmul_rn(alpha, p));
    }
};

// ... the second as one fused multiply-add
struct UpdateFma {
    static constexpr bool kReadE = true, kReadP = true, kWriteE = true, kWriteP = false;
    float decay, alpha;
    __device__ __forceinline__ void operator()(float &e, float &p) const
    {
        e = __fmaf_rn(alpha, p, __fmul_rn(e, decay));
    }
};

struct Swap {
    static constexpr bool kReadE = true, kReadP = true, kWriteE = true, kWriteP = true;
    __device__ __forceinline__ void operator()(float &e, float &p) const
    {
        const float t = e;
        e = p;
        p = t;
    }
};

struct CopyToEma {
    static constexpr bool kReadE = false, kReadP = true, kWriteE = true, kWriteP = false;
    __device__ __forceinline__ void operator()(float &e, float &p) const { e = p; }
};

struct CopyToModel {
    static constexpr bool kReadE = true, kReadP = false, kWriteE = false, kWriteP = true;
    __device__ __forceinline__ void operator()(float &e, float &p) const { p = e; }
};

template <class Op>
__device__ __forceinline__ void one_element(float *e, float *p, const Op &op)
{
    float a = 0.0f, b = 0.0f;
    if (Op::kReadE) a = *e;
    if (Op::kReadP) b = *p;
    op(a, b);
    if (Op::kWriteE) *e = a;
    if (Op::kWriteP) *p = b;
}

template <class Op>
__device__ __forceinline__ void four_elements(float *e, float *p, const Op &op)
{
    f4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
    if (Op::kReadE) a = *reinterpret_cast<const f4 *>(e);
    if (Op::kReadP) b = *reinterpret_cast<const f4 *>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x = a[k], y = b[k];
        op(x, y);
        a[k] = x;
        b[k] = y;
    }
    if (Op::kWriteE) *reinterpret_cast<f4 *>(e) = a;
    if (Op::kWriteP) *reinterpret_cast<f4 *>(p) = b;
}

template <class Op>
__global__ __launch_bounds__(kThreads) void ema_kernel(float *__restrict__ ema, long long n,
                                                       const zira_ema_segment *__restrict__ segments, int n_segments,
                                                       const int32_t *__restrict__ block_segment, long long n_blocks, Op op)
{
    for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long long cs = blk * kChunk;
        const long long ce = cs + kChunk < n ? cs + kChunk : n;
        for (int s = block_segment[blk]; s >= 0 && s < n_segments; ++s) {
            const zira_ema_segment seg = segments[s];
            if (seg.start >= ce) break;
            // the part of this segment inside this block; never outside [cs, ce), whatever the table says
            const long long lo = seg.start > cs ? seg.start : cs;
            const long long hi = seg.start + seg.numel < ce ? seg.start + seg.numel : ce;
            if (hi <= lo) continue;
            float *e = ema + lo;
            float *p = static_cast<float *>(seg.param) + (lo - seg.start);
            const int len = (int)(hi - lo);   // <= kChunk
            // [0, head) one dword per lane, [head, head + 4 nvec) 16 bytes per lane, the rest one dword per lane again
            int head = len, nvec = 0;
            if ((((uintptr_t)e ^ (uintptr_t)p) & 15) == 0) {
                head = (int)(((16 - ((uintptr_t)e & 15)) & 15) >> 2);
                if (head > len) head = len;
                nvec = (len - head) >> 2;
            }
            const int body_end = head + 4 * nvec;
            for (int i = threadIdx.x; i < head; i += kThreads) one_element(e + i, p + i, op);
            for (int v = threadIdx.x; v < nvec; v += kThreads) four_elements(e + head + 4 * v, p + head + 4 * v, op);
            for (int i = body_end + threadIdx.x; i < len; i += kThreads) one_element(e + i, p + i, op);
        }
    }
}

bool served(const float *ema, long long n, const zira_ema_segment *segments, int n_segments, const int32_t *block_segment)
{
    if (n < 1 || n > kMaxN) return false;
    if (!ema || !segments || !block_segment || n_segments < 1) return false;
    return ((uintptr_t)ema & 3) == 0 && ((uintptr_t)segments & 7) == 0 && ((uintptr_t)block_segment & 3) == 0;
}

template <class Op>
int launch(float *ema, long long n, const zira_ema_segment *segments, int n_segments, const int32_t *block_segment, Op op,
           void *stream)
{
    const long long n_blocks = (n + kChunk - 1) / kChunk;
    const unsigned grid = (unsigned)(n_blocks < kMaxGrid ? n_blocks : kMaxGrid);
    hipLaunchKernelGGL(ema_kernel<Op>, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), ema, n, segments,
                       n_segments, block_segment, n_blocks, op);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int zira_ema_update_f32(float *ema, int64_t n, const zira_ema_segment *segments, int n_segments,
                                   const int32_t *block_segment, double decay, double alpha, int contracted, void *stream)
{
    if (!served(ema, n, segments, n_segments, block_segment)) return ZIRA_MSDA_EINVAL;
    if (contracted) return launch(ema, n, segments, n_segments, block_segment, UpdateFma{(float)decay, (float)alpha}, stream);
    return launch(ema, n, segments, n_segments, block_segment, UpdateMulAdd{(float)decay, (float)alpha}, stream);
}

extern "C" int zira_ema_swap_f32(float *ema, int64_t n, const zira_ema_segment *segments, int n_segments,
                                 const int32_t *block_segment, void *stream)
{
    if (!served(ema, n, segments, n_segments, block_segment)) return ZIRA_MSDA_EINVAL;
    return launch(ema, n, segments, n_segments, block_segment, Swap{}, stream);
}

extern "C" int zira_ema_copy_f32(float *ema, int64_t n, const zira_ema_segment *segments, int n_segments,
                                 const int32_t *block_segment, int to_model, void *stream)
{
    if (!served(ema, n, segments, n_segments, block_segment)) return ZIRA_MSDA_EINVAL;
    if (to_model) return launch(ema, n, segments, n_segments, block_segment, CopyToModel{}, stream);
    return launch(ema, n, segments, n_segments, block_segment, CopyToEma{}, stream);
}
