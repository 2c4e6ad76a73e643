// optim_tail.hip -- the training tail on the flat gradient bucket: L2 norm, clip, AdamW and gradient clear as TWO launches
// (C ABI: zira_grad_sqnorm_f32, zira_clip_adamw_f32; contract in include/zira_msda.h).
//
// The bucket's flat index space is cut into blocks of kChunk elements, one 256-thread workgroup each, in both kernels.
//   1. grad_sqnorm_kernel: a workgroup sums the squares of its block -- 16 bytes per lane and load, every lane accumulating
//      in double in a fixed order, lanes and waves joined by lane_sum.h's exchanges and four LDS words -- and stores one double.
//   2. clip_adamw_kernel: EVERY workgroup re-adds all partials (thread t takes partials t, t + 256, ... in index order, then
//      the same lane and wave sums), so all hold the same total bit for bit without any hand-off between workgroups; at the
//      model's 4.6 M values that is 1130 doubles (9 KB, from L2) per workgroup, five loads per thread, which is why there is
//      no third, folding launch.  Then scale, and per element the AdamW update and grad = 0.
// The parameters stay separate tensors: a block finds its segment(s) through block_segment[] and the segment table.  Bucket
// offsets are packed, so a segment starts at any flat offset and the bucket and the parameter differ in phase: 16-byte
// groups are laid on the flat index (multiples of 4), single elements are taken at a segment's two ends, and every 16-byte
// access is typed with 4-byte alignment -- global_load / global_store_dwordx4 on gfx950 need no more than dword alignment,
// so neither the phase difference nor a misaligned bucket forces the scalar path on a segment's body.
// No atomics, no waiting between workgroups; the arithmetic is not contracted, each operation rounds as torch's op chain does.
//
// Under fp16 loss scaling (zira_grad_sqnorm_amp_f32, zira_clip_adamw_amp_f32) the same two launches also do the GradScaler's
// work: kernel 1 takes every element times 1 / scale and notes per block whether a raw value was inf or NaN; every workgroup
// of kernel 2 ORs those flags beside re-adding the partials, so all of them take the same decision -- step, or leave
// parameters and moments alone -- and one thread updates scale, growth tracker and step counter as torch._amp_update_scale_
// does.  The scale and the step count that kernel 2's workgroups compute with are a snapshot kernel 1 wrote into the workspace:
// nobody reads the live values in the launch that writes them.  Both walks are the ones below, instantiated with kAmp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lane_sum.h"
#include "zira_msda.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = ZIRA_OPTIM_TAIL_CHUNK;
constexpr int kMaxGroups = ZIRA_OPTIM_TAIL_MAX_GROUPS;
constexpr long long kMaxN = 1ll << 26;   // 16384 partials: the per-workgroup re-add stays a small share of the kernel
static_assert(kChunk % (4 * kThreads) == 0, "a block is a whole number of 16-byte rounds of the workgroup");

typedef float f4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes, dword aligned

struct Hyper {
    float decay[kMaxGroups];      // 1 - lr wd
    float neg_step[kMaxGroups];   // -lr / bc1
    float w1, b2, w2;             // 1 - beta1, beta2, 1 - beta2
    float bc2_sqrt, eps, max_norm;
    int do_step;
};

__device__ __forceinline__ long long blocks_of(long long n)
{
    return (n + kChunk - 1) / kChunk;
}

// the workgroup's total of one double per thread, the same value in every thread (fixed order: lanes, then waves 0..3)
__device__ __forceinline__ double block_sum(double x, double *lds)
{
    x = lane_sum<64>(x);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += lds[w];
    return t;
}

// a raw gradient times 1 / scale, as _amp_foreach_non_finite_check_and_unscale_ takes it
template <class T>
__device__ __forceinline__ T unscaled(T g, float inv_scale)
{
    return inv_scale == 1.0f ? g : g * inv_scale;
}

__device__ __forceinline__ int non_finite(float x)
{
    return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// the workspace of the amp entries: one double per block, the snapshot, one flag per block
struct AmpSnapshot {
    float scale;
    int32_t step;
    int32_t unused[2];
};

__host__ __device__ __forceinline__ AmpSnapshot *snapshot_of(double *partial, long long blocks)
{
    return reinterpret_cast<AmpSnapshot *>(partial + blocks);
}

__host__ __device__ __forceinline__ int32_t *flags_of(double *partial, long long blocks)
{
    return reinterpret_cast<int32_t *>(partial + blocks + sizeof(AmpSnapshot) / sizeof(double));
}

// this thread's share of the squares of block blockIdx.x; kAmp: of the unscaled values, `bad` noting a non-finite raw one
template <bool kAmp>
__device__ __forceinline__ double thread_sqsum(const float *__restrict__ grad, long long n, float inv_scale, int &bad)
{
    const long long cs = (long long)blockIdx.x * kChunk;
    const long long ce = cs + kChunk < n ? cs + kChunk : n;
    const int len = (int)(ce - cs), nvec = len >> 2;
    const float *g = grad + cs;
    double acc = 0.0;
    for (int v = threadIdx.x; v < nvec; v += kThreads) {
        f4 x = *reinterpret_cast<const f4 *>(g + 4 * v);
        if (kAmp) {
            bad |= non_finite(x.x) | non_finite(x.y) | non_finite(x.z) | non_finite(x.w);
            x = unscaled(x, inv_scale);
        }
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
    }
    const int i = 4 * nvec + (int)threadIdx.x;   // the last block's odd end
    if (i < len) {
        float x = g[i];
        if (kAmp) {
            bad |= non_finite(x);
            x = unscaled(x, inv_scale);
        }
        acc += (double)x * (double)x;
    }
    return acc;
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const float *__restrict__ grad, long long n,
                                                               double *__restrict__ partial)
{
    __shared__ double lds[kWaves];
    int bad = 0;
    const double total = block_sum(thread_sqsum<false>(grad, n, 1.0f, bad), lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_amp_kernel(const float *__restrict__ grad, long long n,
                                                                   const float *__restrict__ scale,
                                                                   const int32_t *__restrict__ step, double *__restrict__ partial)
{
    __shared__ double lds[kWaves];
    const float s = *scale;
    const float inv_scale = (float)(1.0 / (double)s);   // GradScaler: _scale.double().reciprocal().float()
    int bad = 0;
    const double total = block_sum(thread_sqsum<true>(grad, n, inv_scale, bad), lds);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = total;
        flags_of(partial, gridDim.x)[blockIdx.x] = bad ? 1 : 0;
        if (blockIdx.x == 0) *snapshot_of(partial, gridDim.x) = AmpSnapshot{s, *step, {0, 0}};
    }
}

struct Moments {
    float p, m, v;
};

// torch.optim.AdamW's single-tensor update, operation by operation
__device__ __forceinline__ Moments adamw(float p, float g, float m, float v, const Hyper &h, float decay, float neg_step)
{
    Moments o;
    p = p * decay;                                          // param.mul_(1 - lr * weight_decay)
    const float d = g - m;                                  // exp_avg.lerp_(grad, 1 - beta1)
    o.m = h.w1 < 0.5f ? m + h.w1 * d : g - d * (1.0f - h.w1);
    o.v = v * h.b2;                                         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    o.v = o.v + h.w2 * g * g;
    const float denom = sqrtf(o.v) / h.bc2_sqrt + h.eps;    // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    o.p = p + neg_step * (o.m / denom);                     // param.addcdiv_(exp_avg, denom, value=-step_size)
    return o;
}

template <bool kAmp>
__device__ __forceinline__ void one_element(float *grad, float *p, float *m, float *v, float inv_scale, float scale,
                                            const Hyper &h, float decay, float neg_step)
{
    float g = *grad;
    if (kAmp) g = unscaled(g, inv_scale);
    g = g * scale;
    if (!kAmp && !h.do_step) {
        *grad = g;
        return;
    }
    const Moments o = adamw(*p, g, *m, *v, h, decay, neg_step);
    *p = o.p;
    *m = o.m;
    *v = o.v;
    *grad = 0.0f;
}

// the total of the partials, the same bits in every workgroup (thread t takes partials t, t + 256, ... in index order);
// kAmp: `bad` ORs the blocks' flags on the way
template <bool kAmp>
__device__ __forceinline__ float total_norm_of(const double *__restrict__ partial, const int32_t *__restrict__ flags,
                                               int n_partials, double *lds, int &bad)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kThreads) {
        acc += partial[i];
        if (kAmp) bad |= flags[i];
    }
    return (float)sqrt(block_sum(acc, lds));
}

__device__ __forceinline__ float clip_of(float total_norm, float max_norm)
{
    const float q = max_norm / (total_norm + 1e-6f);
    return q > 1.0f ? 1.0f : q;   // (a NaN stays a NaN, as torch.clamp(max=1.0) keeps it)
}

// block blockIdx.x's part of every segment it touches: grad * scale (kAmp: the unscaled grad), AdamW, grad = 0
template <bool kAmp>
__device__ __forceinline__ void walk_block(float *__restrict__ grad, float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                           long long n, const zira_optim_segment *__restrict__ segments, int n_segments,
                                           const int32_t *__restrict__ block_segment, float inv_scale, float scale,
                                           const Hyper &h, const float *decay_of, const float *neg_step_of)
{
    const long long cs = (long long)blockIdx.x * kChunk;
    const long long ce = cs + kChunk < n ? cs + kChunk : n;
    for (int s = block_segment[blockIdx.x]; s >= 0 && s < n_segments; ++s) {
        const zira_optim_segment seg = segments[s];
        if (seg.start >= ce) break;
        // the part of this segment inside this block; never outside [cs, ce), whatever the table says
        const long long lo = seg.start > cs ? seg.start : cs;
        const long long hi = seg.start + seg.numel < ce ? seg.start + seg.numel : ce;
        if (hi <= lo) continue;
        const int grp = (int)seg.group & (kMaxGroups - 1);
        const float decay = decay_of[grp], neg_step = neg_step_of[grp];
        float *p0 = static_cast<float *>(seg.param) - seg.start;   // p0 + flat index = the element
        long long a = (lo + 3) & ~3ll;                              // 16-byte groups on multiples of 4 of the flat index
        if (a > hi) a = hi;
        const int head = (int)(a - lo), nvec = (int)((hi - a) >> 2);
        const long long b = a + 4ll * nvec;
        const int tail = (int)(hi - b);
        if ((int)threadIdx.x < head) {
            const long long i = lo + threadIdx.x;
            one_element<kAmp>(grad + i, p0 + i, exp_avg + i, exp_avg_sq + i, inv_scale, scale, h, decay, neg_step);
        }
        if (!kAmp && !h.do_step) {
            for (int v = threadIdx.x; v < nvec; v += kThreads) {
                f4 *g = reinterpret_cast<f4 *>(grad + a + 4ll * v);
                *g = *g * scale;
            }
        } else {
            for (int v = threadIdx.x; v < nvec; v += kThreads) {
                const long long i = a + 4ll * v;
                f4 g = *reinterpret_cast<const f4 *>(grad + i);   // (four loads in flight, then the arithmetic)
                if (kAmp) g = unscaled(g, inv_scale);
                g = g * scale;
                f4 p = *reinterpret_cast<const f4 *>(p0 + i);
                f4 m = *reinterpret_cast<const f4 *>(exp_avg + i);
                f4 w = *reinterpret_cast<const f4 *>(exp_avg_sq + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const Moments o = adamw(p[k], g[k], m[k], w[k], h, decay, neg_step);
                    p[k] = o.p;
                    m[k] = o.m;
                    w[k] = o.v;
                }
                *reinterpret_cast<f4 *>(p0 + i) = p;
                *reinterpret_cast<f4 *>(exp_avg + i) = m;
                *reinterpret_cast<f4 *>(exp_avg_sq + i) = w;
                *reinterpret_cast<f4 *>(grad + i) = f4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        if ((int)threadIdx.x < tail) {
            const long long i = b + threadIdx.x;
            one_element<kAmp>(grad + i, p0 + i, exp_avg + i, exp_avg_sq + i, inv_scale, scale, h, decay, neg_step);
        }
    }
}

__global__ __launch_bounds__(kThreads) void clip_adamw_kernel(float *__restrict__ grad, float *__restrict__ exp_avg,
                                                              float *__restrict__ exp_avg_sq, long long n,
                                                              const zira_optim_segment *__restrict__ segments, int n_segments,
                                                              const int32_t *__restrict__ block_segment,
                                                              const double *__restrict__ partial, float *__restrict__ norm_out,
                                                              Hyper h)
{
    __shared__ double lds[kWaves];
    int bad = 0;
    const float total_norm = total_norm_of<false>(partial, nullptr, (int)blocks_of(n), lds, bad);
    const float scale = clip_of(total_norm, h.max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total_norm;
    walk_block<false>(grad, exp_avg, exp_avg_sq, n, segments, n_segments, block_segment, 1.0f, scale, h, h.decay, h.neg_step);
}

// what the amp kernel needs beside Hyper: the step-dependent factors are formed on the device, the scaler's state is updated
struct AmpArgs {
    double lrs[kMaxGroups];
    double beta1, beta2, growth_factor, backoff_factor;
    float *scale;
    int32_t *growth_tracker, *step;
    float *found_inf_out;
    int n_groups, growth_interval;
};

// torch._amp_update_scale_, line for line, from the snapshot's scale; one thread of the launch
__device__ __forceinline__ void update_scale(const AmpArgs &a, float scale, int found_inf)
{
    if (found_inf) {
        *a.scale = (float)(scale * a.backoff_factor);
        *a.growth_tracker = 0;
        return;
    }
    const int32_t successful = *a.growth_tracker + 1;
    if (successful == a.growth_interval) {
        const float grown = (float)(scale * a.growth_factor);
        if (!non_finite(grown)) *a.scale = grown;
        *a.growth_tracker = 0;
    } else {
        *a.growth_tracker = successful;
    }
}

__global__ __launch_bounds__(kThreads) void clip_adamw_amp_kernel(float *__restrict__ grad, float *__restrict__ exp_avg,
                                                                  float *__restrict__ exp_avg_sq, long long n,
                                                                  const zira_optim_segment *__restrict__ segments,
                                                                  int n_segments, const int32_t *__restrict__ block_segment,
                                                                  double *__restrict__ ws, float *__restrict__ norm_out, Hyper h,
                                                                  AmpArgs a)
{
    __shared__ double lds[kWaves];
    __shared__ float neg_step_of[kMaxGroups];
    __shared__ float bc2_sqrt;
    const int n_partials = (int)blocks_of(n);
    const AmpSnapshot snap = *snapshot_of(ws, n_partials);
    int bad = 0;
    const float total_norm = total_norm_of<true>(ws, flags_of(ws, n_partials), n_partials, lds, bad);
    bad = __syncthreads_or(bad);
    const int t = snap.step + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *norm_out = total_norm;
        *a.found_inf_out = bad ? 1.0f : 0.0f;
        update_scale(a, snap.scale, bad);
        if (!bad) *a.step = t;
    }
    if (bad) {   // the skipped step: the bucket is cleared, nothing else of the model is touched
        const long long cs = (long long)blockIdx.x * kChunk;
        const long long ce = cs + kChunk < n ? cs + kChunk : n;
        const int len = (int)(ce - cs), nvec = len >> 2;
        for (int v = threadIdx.x; v < nvec; v += kThreads)
            *reinterpret_cast<f4 *>(grad + cs + 4 * v) = f4{0.0f, 0.0f, 0.0f, 0.0f};
        const int i = 4 * nvec + (int)threadIdx.x;
        if (i < len) grad[cs + i] = 0.0f;
        return;
    }
    // the bias corrections of step t, once per workgroup: one lane per learning-rate group
    if (threadIdx.x < kMaxGroups) {
        const double bc1 = 1.0 - pow(a.beta1, (double)t);
        neg_step_of[threadIdx.x] = (int)threadIdx.x < a.n_groups ? (float)(-(a.lrs[threadIdx.x] / bc1)) : 0.0f;
        if (threadIdx.x == 0) bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2, (double)t));
    }
    __syncthreads();
    h.bc2_sqrt = bc2_sqrt;
    const float inv_scale = (float)(1.0 / (double)snap.scale);
    walk_block<true>(grad, exp_avg, exp_avg_sq, n, segments, n_segments, block_segment, inv_scale, clip_of(total_norm, h.max_norm),
                     h, h.decay, neg_step_of);
}

bool served(long long n)
{
    return n >= 1 && n <= kMaxN;
}

size_t workspace_bytes(long long n)
{
    return (size_t)((n + kChunk - 1) / kChunk) * sizeof(double);
}

size_t amp_workspace_bytes(long long n)
{
    const size_t blocks = (size_t)((n + kChunk - 1) / kChunk);
    return blocks * sizeof(double) + sizeof(AmpSnapshot) + (blocks + 1) / 2 * 2 * sizeof(int32_t);
}

// the step's constants as torch.optim.AdamW's single-tensor path rounds them
bool fill_hyper(Hyper &h, const double *lrs, int n_groups, double beta1, double beta2, double eps, double weight_decay, double bc1,
                double bc2_sqrt)
{
    if (!lrs || n_groups < 1 || n_groups > kMaxGroups) return false;
    for (int g = 0; g < n_groups; ++g) {
        h.decay[g] = (float)(1.0 - lrs[g] * weight_decay);
        h.neg_step[g] = (float)(-(lrs[g] / bc1));
    }
    h.w1 = (float)(1.0 - beta1);
    h.b2 = (float)beta2;
    h.w2 = (float)(1.0 - beta2);
    h.bc2_sqrt = (float)bc2_sqrt;
    h.eps = (float)eps;
    return true;
}

}  // namespace

extern "C" size_t zira_optim_tail_workspace_bytes(int64_t n)
{
    return served(n) ? workspace_bytes(n) : 0;
}

extern "C" size_t zira_optim_tail_amp_workspace_bytes(int64_t n)
{
    return served(n) ? amp_workspace_bytes(n) : 0;
}

extern "C" int zira_grad_sqnorm_f32(const float *grad, int64_t n, void *ws, size_t ws_bytes, void *stream)
{
    if (!grad || !ws || !served(n) || ws_bytes < workspace_bytes(n)) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)grad & 3) || ((uintptr_t)ws & 7)) return ZIRA_MSDA_EINVAL;
    const unsigned blocks = (unsigned)(workspace_bytes(n) / sizeof(double));
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad, (long long)n,
                       static_cast<double *>(ws));
    return (int)hipGetLastError();
}

extern "C" int zira_grad_sqnorm_amp_f32(const float *grad, int64_t n, const float *scale, const int32_t *step, void *ws,
                                        size_t ws_bytes, void *stream)
{
    if (!grad || !scale || !step || !ws || !served(n) || ws_bytes < amp_workspace_bytes(n)) return ZIRA_MSDA_EINVAL;
    if ((((uintptr_t)grad | (uintptr_t)scale | (uintptr_t)step) & 3) || ((uintptr_t)ws & 7)) return ZIRA_MSDA_EINVAL;
    const unsigned blocks = (unsigned)(workspace_bytes(n) / sizeof(double));
    hipLaunchKernelGGL(grad_sqnorm_amp_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad,
                       (long long)n, scale, step, static_cast<double *>(ws));
    return (int)hipGetLastError();
}

extern "C" int zira_clip_adamw_f32(float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const zira_optim_segment *segments,
                                   int n_segments, const int32_t *block_segment, const double *lrs, int n_groups, double beta1,
                                   double beta2, double eps, double weight_decay, double bc1, double bc2, double bc2_sqrt,
                                   double max_norm, int do_step, float *norm_out, const void *ws, size_t ws_bytes, void *stream)
{
    if (!grad || !norm_out || !ws || !served(n) || ws_bytes < workspace_bytes(n)) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)grad & 3) || ((uintptr_t)norm_out & 3) || ((uintptr_t)ws & 7)) return ZIRA_MSDA_EINVAL;
    if (!segments || n_segments < 1 || !block_segment) return ZIRA_MSDA_EINVAL;
    Hyper h = {};
    h.max_norm = (float)max_norm;
    h.do_step = do_step ? 1 : 0;
    if (do_step) {
        if (!exp_avg || !exp_avg_sq) return ZIRA_MSDA_EINVAL;
        if (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3) return ZIRA_MSDA_EINVAL;
        if (!(bc1 > 0.0) || !(bc2 > 0.0) || !(bc2_sqrt > 0.0)) return ZIRA_MSDA_EINVAL;
        if (!fill_hyper(h, lrs, n_groups, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt)) return ZIRA_MSDA_EINVAL;
    }
    const unsigned blocks = (unsigned)(workspace_bytes(n) / sizeof(double));
    hipLaunchKernelGGL(clip_adamw_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad, exp_avg,
                       exp_avg_sq, (long long)n, segments, n_segments, block_segment, static_cast<const double *>(ws), norm_out, h);
    return (int)hipGetLastError();
}

extern "C" int zira_clip_adamw_amp_f32(float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                       const zira_optim_segment *segments, int n_segments, const int32_t *block_segment,
                                       const double *lrs, int n_groups, double beta1, double beta2, double eps,
                                       double weight_decay, double max_norm, float *scale, int32_t *growth_tracker, int32_t *step,
                                       double growth_factor, double backoff_factor, int growth_interval, float *norm_out,
                                       float *found_inf_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!grad || !exp_avg || !exp_avg_sq || !norm_out || !found_inf_out || !scale || !growth_tracker || !step || !ws)
        return ZIRA_MSDA_EINVAL;
    if (!served(n) || ws_bytes < amp_workspace_bytes(n)) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)norm_out | (uintptr_t)found_inf_out |
         (uintptr_t)scale | (uintptr_t)growth_tracker | (uintptr_t)step) & 3)
        return ZIRA_MSDA_EINVAL;
    if ((uintptr_t)ws & 7) return ZIRA_MSDA_EINVAL;
    if (!segments || n_segments < 1 || !block_segment) return ZIRA_MSDA_EINVAL;
    if (growth_interval < 1 || !(growth_factor > 0.0) || !(backoff_factor > 0.0)) return ZIRA_MSDA_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return ZIRA_MSDA_EINVAL;   // (bc1, bc2 > 0 at every step)
    Hyper h = {};
    h.max_norm = (float)max_norm;
    h.do_step = 1;
    if (!fill_hyper(h, lrs, n_groups, beta1, beta2, eps, weight_decay, 1.0, 1.0)) return ZIRA_MSDA_EINVAL;   // (bc: the kernel's)
    AmpArgs a = {};
    for (int g = 0; g < n_groups; ++g) a.lrs[g] = lrs[g];
    a.beta1 = beta1, a.beta2 = beta2, a.growth_factor = growth_factor, a.backoff_factor = backoff_factor;
    a.scale = scale, a.growth_tracker = growth_tracker, a.step = step, a.found_inf_out = found_inf_out;
    a.n_groups = n_groups, a.growth_interval = growth_interval;
    const unsigned blocks = (unsigned)(workspace_bytes(n) / sizeof(double));
    hipLaunchKernelGGL(clip_adamw_amp_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad, exp_avg,
                       exp_avg_sq, (long long)n, segments, n_segments, block_segment, static_cast<double *>(ws), norm_out, h, a);
    return (int)hipGetLastError();
}
