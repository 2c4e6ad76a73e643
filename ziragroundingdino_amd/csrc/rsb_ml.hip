// rsb_ml.hip -- fused epilogue of the multilayer-branch ZiRa side branches for gfx950 (MI355X), float32.
//
// Reference semantics (models/GroundingDINO/groundingdino_dual_zero_rep_multilayer_branch.py, training mode):
//   RepZeroLinear.forward (:116-146)     branch = scaling * F(x; W, b);  out = branch + F(x; W_f, b_f)
//                                        loss   = mean|branch| + mean|out|                       (nn.L1Loss to zero)
//   RepZeroConv2dGN.forward (:69-113)    out    = GroupNorm_{gamma, beta}(branch + twin), gamma and beta TRAINED
//                                        loss   = mean|branch| + mean|out|
// The two contractions stay with the GEMM library; everything after them is here (C ABI and formulas: include/zira_rsb_ml.h).
//
// Language branch: one grid-stride pass each way, as csrc/rsb.hip, and a one-block finish.
//
// Vision branch: the unit of work is a PART of a channel row, (b, c, p): HW / S contiguous floats of one channel.  A channel,
// not a (sample, group) run as in csrc/groupnorm.hip, because gamma and beta are trained: the sums g_gamma_c and g_beta_c
// are per channel, and a block that stays inside one channel keeps them in two registers.  S is chosen so that a launch has
// about 256 CUs x 8 blocks while a part keeps at least 1024 floats (one float4 per thread): S = 4 at the model's first level
// (2 x 256 x 16700), 1 at the last (2 x 256 x 273).  HW may be odd, so a part starts at any alignment: up to three scalar
// elements, the float4 body, up to three scalar elements.
//   forward   k1: per block the sum of x, then -- the part is read again, from L2 -- the squared distances to the block's
//                 own mean, and sum|branch|;  k2: every block joins the (C / G) * S records of its group (exact in double,
//                 record order: the same bits in every block of the group), normalises its part, sums |out|;  k3: loss.
//   backward  k1: per block sum(dout) and sum(dout * xhat);  k2: the group's two means from those records and gamma, then
//                 dx, g_branch, g_twin and the block's sum(y_branch * d);  k3: g_gamma, g_beta (a block per channel, over
//                 b and p) and g_scaling.
// HBM-bound: forward 2 reads (+ 2 from L2) + 2 reads + 1 write per element, backward 4 reads + 4 reads + 2 writes.
//
// Every sum is carried in double from the thread's accumulator on, written per block to the workspace and folded in a fixed
// order: no atomics, no arrival counters, the same bits on every run.  The backward's element arithmetic is in double as well
// (dx is a difference of three terms of like size and feeds the three parameter sums; the results are rounded to float
// once, when stored): about twenty fp64 instructions per element, a tenth of the time the 16 to 24 bytes per element take.

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lane_sum.h"
#include "launch.h"
#include "zira_rsb_ml.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;      // 256 CUs x 8
constexpr long kMinPart = 1024;       // floats: one float4 per thread
constexpr int kMaxSplit = 64;

template <int W>
struct Width {
    static constexpr int value = W;
};

template <int W>
__device__ __forceinline__ void ld(const float *p, long i, float (&v)[4])
{
    if (W == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[i];
    }
}

template <int W>
__device__ __forceinline__ void st(float *p, long i, const float (&v)[4])
{
    if (W == 4)
        *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    else
        p[i] = v[0];
}

// f(Width<1 or 4>, i) for the elements [beg, end) of 16-byte aligned arrays, dealt to `stride` threads of which this is
// number `first`: scalars up to the first multiple of 4, float4s, scalars behind the last whole float4
template <class F>
__device__ __forceinline__ void for_span(long beg, long end, long first, long stride, F &&f)
{
    long head = (beg + 3) & ~3l;
    if (head > end) head = end;
    const long body_end = head + ((end - head) & ~3l);
    if (beg + first < head) f(Width<1>(), beg + first);
    for (long i = head + 4 * first; i < body_end; i += 4 * stride) f(Width<4>(), i);
    if (body_end + first < end) f(Width<1>(), body_end + first);
}

__device__ __forceinline__ double sgn(double t) { return (double)((t > 0.0) - (t < 0.0)); }      // sign(0) = 0, as autograd's abs

// block-wide sums of NV doubles, every thread receives them; waves in a fixed order
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double (*red)[kWaves])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                       // (red may still be read from the previous call)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = lane_sum<64>(v[i]);
        if (lane == 0) red[i][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

// d/dloss of one element of a mean over n
__device__ __forceinline__ double loss_grad(const float *grad_loss, double n)
{
    return grad_loss ? (double)grad_loss[0] / n : 0.0;
}

// ---- language branch ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void l1_fwd_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                         const float *__restrict__ scaling, long n, float *__restrict__ out,
                                                         double *__restrict__ partial)
{
    __shared__ double red[2][kWaves];
    const float s = scaling[0];
    double acc[2] = {0.0, 0.0};
    for_span(0, n, (long)blockIdx.x * kThreads + threadIdx.x, (long)gridDim.x * kThreads, [&](auto w, long i) {
        constexpr int W = decltype(w)::value;
        float b[4], t[4], o[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            o[e] = __fmaf_rn(s, b[e], t[e]);
            acc[0] += (double)fabsf(s * b[e]);
            acc[1] += (double)fabsf(o[e]);
        }
        st<W>(out, i, o);
    });
    block_sum_d<2>(acc, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = acc[0];
        partial[2 * blockIdx.x + 1] = acc[1];
    }
}

// loss = sum(partial[.][0]) / n + sum(partial[.][1]) / n; the records lie `stride` doubles apart
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(const double *__restrict__ pa, int stride_a, const double *__restrict__ pb,
                                                              int stride_b, long nblocks, double n, float *__restrict__ loss)
{
    __shared__ double red[2][kWaves];
    double acc[2] = {0.0, 0.0};
    for (long i = threadIdx.x; i < nblocks; i += kThreads) {
        acc[0] += pa[i * stride_a];
        acc[1] += pb[i * stride_b];
    }
    block_sum_d<2>(acc, red);
    if (threadIdx.x == 0) loss[0] = (float)(acc[0] / n + acc[1] / n);
}

__global__ __launch_bounds__(kThreads) void l1_bwd_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                         const float *__restrict__ scaling, const float *__restrict__ grad_out,
                                                         const float *__restrict__ grad_loss, long n, float *__restrict__ g_yb,
                                                         float *__restrict__ g_yt, double *__restrict__ partial)
{
    __shared__ double red[1][kWaves];
    const float s = scaling[0];
    const double gl = loss_grad(grad_loss, (double)n);
    double acc[1] = {0.0};
    for_span(0, n, (long)blockIdx.x * kThreads + threadIdx.x, (long)gridDim.x * kThreads, [&](auto w, long i) {
        constexpr int W = decltype(w)::value;
        float b[4], t[4], go[4] = {0.f, 0.f, 0.f, 0.f}, gb[4], gt[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
        if (grad_out) ld<W>(grad_out, i, go);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const double br = (double)s * (double)b[e];
            const double d_out = (double)go[e] + gl * sgn((double)__fmaf_rn(s, b[e], t[e]));
            const double d = d_out + gl * sgn(br);
            gt[e] = (float)d_out;
            gb[e] = (float)((double)s * d);
            acc[0] += (double)b[e] * d;
        }
        st<W>(g_yb, i, gb);
        st<W>(g_yt, i, gt);
    });
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(kThreads) void scalar_finish_kernel(const double *__restrict__ partial, long nblocks,
                                                                float *__restrict__ dst)
{
    __shared__ double red[1][kWaves];
    double acc[1] = {0.0};
    for (long i = threadIdx.x; i < nblocks; i += kThreads) acc[0] += partial[i];
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) dst[0] = (float)acc[0];
}

inline int l1_grid(size_t n)
{
    size_t blocks = ((n >> 2) + kThreads - 1) / kThreads;
    blocks = blocks < 1 ? 1 : (blocks > (size_t)kMaxBlocks ? (size_t)kMaxBlocks : blocks);
    return (int)blocks;
}

// ---- vision branch -----------------------------------------------------------------------------------------------------------------
struct Geom {
    int C, HW, G, cpg, S;
    long part;      // floats of a part, a multiple of 4; the last part of a row may be shorter
    long blocks;    // B * C * S
    double run;     // elements of a (sample, group): cpg * HW
};

// the block's part of its channel row and the records of its group
struct Where {
    long beg, end;      // elements of the tensor
    int c, bg;          // channel; b * G + group
    long first;         // the group's records are first .. first + cpg * S, channel-major
    bool leads;         // the group's first block
};

__device__ __forceinline__ long part_len(const Geom &g, int p)
{
    const long a = (long)p * g.part, b = a + g.part;
    return (b < g.HW ? b : (long)g.HW) - (a < g.HW ? a : (long)g.HW);
}

__device__ __forceinline__ Where where(const Geom &g)
{
    Where w;
    const long row = blockIdx.x / g.S;
    const int p = (int)(blockIdx.x - row * g.S);
    const long a = (long)p * g.part;
    w.beg = row * g.HW + (a < g.HW ? a : (long)g.HW);
    w.end = w.beg + part_len(g, p);
    const long b = row / g.C;
    w.c = (int)(row - b * g.C);
    const int grp = w.c / g.cpg;
    w.bg = (int)(b * g.G + grp);
    w.first = (b * g.C + (long)grp * g.cpg) * g.S;
    w.leads = p == 0 && w.c == grp * g.cpg;
    return w;
}

// k1 of the forward: record {sum x, m, sum (x - m)^2, sum |branch|} with m the block's own mean rounded to float
__global__ __launch_bounds__(kThreads) void gn_stats_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                           const float *__restrict__ scaling, Geom g, double *__restrict__ rec)
{
    __shared__ double red[2][kWaves];
    const Where w = where(g);
    const float s = scaling[0];
    double acc[2] = {0.0, 0.0};
    for_span(w.beg, w.end, threadIdx.x, kThreads, [&](auto wd, long i) {
        constexpr int W = decltype(wd)::value;
        float b[4], t[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            acc[0] += (double)__fmaf_rn(s, b[e], t[e]);
            acc[1] += (double)fabsf(s * b[e]);
        }
    });
    block_sum_d<2>(acc, red);
    const long n = w.end - w.beg;
    const float m = n > 0 ? (float)(acc[0] / (double)n) : 0.f;
    double q[1] = {0.0};
    for_span(w.beg, w.end, threadIdx.x, kThreads, [&](auto wd, long i) {
        constexpr int W = decltype(wd)::value;
        float b[4], t[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const double d = (double)__fmaf_rn(s, b[e], t[e]) - (double)m;
            q[0] += d * d;
        }
    });
    block_sum_d<1>(q, red);
    if (threadIdx.x == 0) {
        double *o = rec + (size_t)blockIdx.x * 4;
        o[0] = acc[0]; o[1] = (double)m; o[2] = q[0]; o[3] = acc[1];
    }
}

// mean and rstd of the block's group from its cpg * S records: mu = sum(sum_j) / run, and around mu
//   sum (x - mu)^2 = sum_j [ q_j + 2 (m_j - mu) (sum_j - n_j m_j) + n_j (m_j - mu)^2 ]      (exact, whatever m_j is)
__device__ __forceinline__ void join_stats(const Geom &g, const Where &w, const double *rec, float eps, double (*red)[kWaves],
                                           float &mean, float &rstd)
{
    const int P = g.cpg * g.S;
    double a[1] = {0.0};
    for (int j = threadIdx.x; j < P; j += kThreads) a[0] += rec[(size_t)(w.first + j) * 4];
    block_sum_d<1>(a, red);
    const double mu = a[0] / g.run;
    double q[1] = {0.0};
    for (int j = threadIdx.x; j < P; j += kThreads) {
        const double *r = rec + (size_t)(w.first + j) * 4;
        const double n = (double)part_len(g, j % g.S), dm = r[1] - mu;
        q[0] += r[2] + 2.0 * dm * (r[0] - n * r[1]) + n * dm * dm;
    }
    block_sum_d<1>(q, red);
    const double var = q[0] > 0.0 ? q[0] / g.run : 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// k2 of the forward
__global__ __launch_bounds__(kThreads) void gn_norm_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                          const float *__restrict__ scaling, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, Geom g, float eps,
                                                          const double *__restrict__ rec, float *__restrict__ out,
                                                          float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                          double *__restrict__ abs_out)
{
    __shared__ double red[1][kWaves];
    const Where w = where(g);
    float mean, rstd;
    join_stats(g, w, rec, eps, red, mean, rstd);
    if (w.leads && threadIdx.x == 0) {
        mean_out[w.bg] = mean;
        rstd_out[w.bg] = rstd;
    }
    const float s = scaling[0], gam = gamma[w.c], bet = beta[w.c];
    double acc[1] = {0.0};
    for_span(w.beg, w.end, threadIdx.x, kThreads, [&](auto wd, long i) {
        constexpr int W = decltype(wd)::value;
        float b[4], t[4], o[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            o[e] = (__fmaf_rn(s, b[e], t[e]) - mean) * rstd * gam + bet;
            acc[0] += (double)fabsf(o[e]);
        }
        st<W>(out, i, o);
    });
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) abs_out[blockIdx.x] = acc[0];
}

// k1 of the backward: record {sum dout, sum dout * xhat}
__global__ __launch_bounds__(kThreads) void gn_bwd_sums_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                              const float *__restrict__ scaling, const float *__restrict__ mean,
                                                              const float *__restrict__ rstd, const float *__restrict__ out,
                                                              const float *__restrict__ grad_out,
                                                              const float *__restrict__ grad_loss, Geom g, double n_all,
                                                              double *__restrict__ rec)
{
    __shared__ double red[2][kWaves];
    const Where w = where(g);
    const float s = scaling[0];
    const double mu = mean[w.bg], rs = rstd[w.bg];
    const double gl = loss_grad(grad_loss, n_all);
    double acc[2] = {0.0, 0.0};
    for_span(w.beg, w.end, threadIdx.x, kThreads, [&](auto wd, long i) {
        constexpr int W = decltype(wd)::value;
        float b[4], t[4], o[4], go[4] = {0.f, 0.f, 0.f, 0.f};
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
        ld<W>(out, i, o);
        if (grad_out) ld<W>(grad_out, i, go);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const double xh = ((double)__fmaf_rn(s, b[e], t[e]) - mu) * rs;      // the x the statistics were taken from
            const double dout = (double)go[e] + gl * sgn((double)o[e]);
            acc[0] += dout;
            acc[1] += dout * xh;
        }
    });
    block_sum_d<2>(acc, red);
    if (threadIdx.x == 0) {
        rec[(size_t)blockIdx.x * 2] = acc[0];
        rec[(size_t)blockIdx.x * 2 + 1] = acc[1];
    }
}

// k2 of the backward
__global__ __launch_bounds__(kThreads) void gn_bwd_dx_kernel(const float *__restrict__ yb, const float *__restrict__ yt,
                                                            const float *__restrict__ scaling, const float *__restrict__ gamma,
                                                            const float *__restrict__ mean, const float *__restrict__ rstd,
                                                            const float *__restrict__ out, const float *__restrict__ grad_out,
                                                            const float *__restrict__ grad_loss, Geom g, double n_all,
                                                            const double *__restrict__ rec, float *__restrict__ g_yb,
                                                            float *__restrict__ g_yt, double *__restrict__ ysum)
{
    __shared__ double red[2][kWaves];
    const Where w = where(g);
    // mean_group(dout gamma) and mean_group(dout gamma xhat): the channel sums of k1, weighted, in record order
    const int P = g.cpg * g.S, c0 = w.c - w.c % g.cpg;
    double a[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < P; j += kThreads) {
        const double wgt = (double)gamma[c0 + j / g.S];
        a[0] += wgt * rec[(size_t)(w.first + j) * 2];
        a[1] += wgt * rec[(size_t)(w.first + j) * 2 + 1];
    }
    block_sum_d<2>(a, red);
    const double m1 = a[0] / g.run, m2 = a[1] / g.run;
    const float s = scaling[0];
    const double gam = gamma[w.c], mu = mean[w.bg], rs = rstd[w.bg];
    const double gl = loss_grad(grad_loss, n_all);
    double acc[1] = {0.0};
    for_span(w.beg, w.end, threadIdx.x, kThreads, [&](auto wd, long i) {
        constexpr int W = decltype(wd)::value;
        float b[4], t[4], o[4], go[4] = {0.f, 0.f, 0.f, 0.f}, gb[4], gt[4];
        ld<W>(yb, i, b);
        ld<W>(yt, i, t);
        ld<W>(out, i, o);
        if (grad_out) ld<W>(grad_out, i, go);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const double xh = ((double)__fmaf_rn(s, b[e], t[e]) - mu) * rs;
            const double dout = (double)go[e] + gl * sgn((double)o[e]);
            const double dx = rs * (dout * gam - m1 - xh * m2);
            const double d = dx + gl * sgn((double)s * (double)b[e]);
            gt[e] = (float)dx;
            gb[e] = (float)((double)s * d);
            acc[0] += (double)b[e] * d;
        }
        st<W>(g_yb, i, gb);
        if (g_yt) st<W>(g_yt, i, gt);
    });
    block_sum_d<1>(acc, red);
    if (threadIdx.x == 0) ysum[blockIdx.x] = acc[0];
}

// k3 of the backward: block c < C folds channel c's records over b and p; block C folds sum(y_branch * d)
__global__ __launch_bounds__(kThreads) void gn_bwd_finish_kernel(const double *__restrict__ rec, const double *__restrict__ ysum, int B,
                                                                Geom g, float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                                float *__restrict__ g_scaling)
{
    __shared__ double red[2][kWaves];
    double acc[2] = {0.0, 0.0};
    if ((int)blockIdx.x < g.C) {
        const long per = (long)B * g.S;
        for (long j = threadIdx.x; j < per; j += kThreads) {
            const long b = j / g.S, p = j - b * g.S;
            const size_t at = (size_t)((b * g.C + blockIdx.x) * g.S + p) * 2;
            acc[0] += rec[at];
            acc[1] += rec[at + 1];
        }
        block_sum_d<2>(acc, red);
        if (threadIdx.x == 0) {
            g_beta[blockIdx.x] = (float)acc[0];
            g_gamma[blockIdx.x] = (float)acc[1];
        }
    } else {
        for (long j = threadIdx.x; j < g.blocks; j += kThreads) acc[0] += ysum[j];
        block_sum_d<2>(acc, red);
        if (threadIdx.x == 0) g_scaling[0] = (float)acc[0];
    }
}

inline bool make_geom(int B, int C, int HW, int G, Geom &g)
{
    if (B <= 0 || C <= 0 || HW <= 0 || G <= 0 || C % G || (long)B * C > (1l << 20) || HW > (1 << 28)) return false;
    const long rows = (long)B * C;
    long S = (kMaxBlocks + rows - 1) / rows;
    if (S > HW / kMinPart) S = HW / kMinPart;
    S = S < 1 ? 1 : (S > kMaxSplit ? kMaxSplit : S);
    g.C = C; g.HW = HW; g.G = G; g.cpg = C / G; g.S = (int)S;
    g.part = ((HW + S - 1) / S + 3) / 4 * 4;
    g.blocks = rows * S;
    g.run = (double)g.cpg * (double)HW;
    return true;
}

using zira::misaligned;

}  // namespace

extern "C" {

size_t zira_rsb_l1_workspace_floats(size_t n) { return n ? (size_t)kMaxBlocks * 2 * 2 : 0; }

int zira_rsb_l1_fwd_f32(const float *y_branch, const float *y_twin, const float *scaling, size_t n, float *out, float *loss,
                        float *workspace, void *stream)
{
    if (!y_branch || !y_twin || !scaling || !out || !loss || !workspace || n == 0 || n > ((size_t)1 << 40) ||
        misaligned(y_branch, 16) || misaligned(y_twin, 16) || misaligned(out, 16) || misaligned(workspace, 8))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    double *partial = reinterpret_cast<double *>(workspace);
    const int grid = l1_grid(n);
    hipLaunchKernelGGL(l1_fwd_kernel, dim3(grid), dim3(kThreads), 0, st, y_branch, y_twin, scaling, (long)n, out, partial);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, 2, partial + 1, 2, (long)grid, (double)n, loss);
    return (int)hipGetLastError();
}

int zira_rsb_l1_bwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *grad_out,
                        const float *grad_loss, size_t n, float *g_branch, float *g_twin, float *g_scaling, float *workspace,
                        void *stream)
{
    if (!y_branch || !y_twin || !scaling || !g_branch || !g_twin || !g_scaling || !workspace || n == 0 || n > ((size_t)1 << 40) ||
        misaligned(y_branch, 16) || misaligned(y_twin, 16) || misaligned(g_branch, 16) || misaligned(g_twin, 16) ||
        misaligned(grad_out, 16) || misaligned(workspace, 8))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    double *partial = reinterpret_cast<double *>(workspace);
    const int grid = l1_grid(n);
    hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid), dim3(kThreads), 0, st, y_branch, y_twin, scaling, grad_out, grad_loss, (long)n,
                       g_branch, g_twin, partial);
    hipLaunchKernelGGL(scalar_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, (long)grid, g_scaling);
    return (int)hipGetLastError();
}

// forward: 4 doubles of statistics and 1 of sum|out| per block; backward: 2 of channel sums and 1 of sum(y_branch * d)
size_t zira_rsb_gn_workspace_floats(int B, int C, int HW, int G)
{
    Geom g;
    if (!make_geom(B, C, HW, G, g)) return 0;
    return (size_t)g.blocks * 5 * 2;
}

int zira_rsb_gn_fwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *gamma, const float *beta,
                        int B, int C, int HW, int G, float eps, float *out, float *loss, float *mean, float *rstd,
                        float *workspace, void *stream)
{
    Geom g;
    if (!y_branch || !y_twin || !scaling || !gamma || !beta || !out || !loss || !mean || !rstd || !workspace ||
        !make_geom(B, C, HW, G, g) || misaligned(y_branch, 16) || misaligned(y_twin, 16) || misaligned(out, 16) ||
        misaligned(workspace, 8))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    double *rec = reinterpret_cast<double *>(workspace), *abs_out = rec + (size_t)g.blocks * 4;
    const dim3 grid((unsigned)g.blocks);
    hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(kThreads), 0, st, y_branch, y_twin, scaling, g, rec);
    hipLaunchKernelGGL(gn_norm_kernel, grid, dim3(kThreads), 0, st, y_branch, y_twin, scaling, gamma, beta, g, eps, rec, out, mean,
                       rstd, abs_out);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, rec + 3, 4, abs_out, 1, g.blocks,
                       (double)B * (double)C * (double)HW, loss);
    return (int)hipGetLastError();
}

int zira_rsb_gn_bwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *gamma, const float *mean,
                        const float *rstd, const float *out, const float *grad_out, const float *grad_loss, int B, int C, int HW,
                        int G, float *g_branch, float *g_twin, float *g_scaling, float *g_gamma, float *g_beta, float *workspace,
                        void *stream)
{
    Geom g;
    if (!y_branch || !y_twin || !scaling || !gamma || !mean || !rstd || !out || !g_branch || !g_scaling || !g_gamma || !g_beta ||
        !workspace || !make_geom(B, C, HW, G, g) || misaligned(y_branch, 16) || misaligned(y_twin, 16) || misaligned(out, 16) ||
        misaligned(grad_out, 16) || misaligned(g_branch, 16) || misaligned(g_twin, 16) || misaligned(workspace, 8))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    double *rec = reinterpret_cast<double *>(workspace), *ysum = rec + (size_t)g.blocks * 2;
    const double n_all = (double)B * (double)C * (double)HW;
    const dim3 grid((unsigned)g.blocks);
    hipLaunchKernelGGL(gn_bwd_sums_kernel, grid, dim3(kThreads), 0, st, y_branch, y_twin, scaling, mean, rstd, out, grad_out,
                       grad_loss, g, n_all, rec);
    hipLaunchKernelGGL(gn_bwd_dx_kernel, grid, dim3(kThreads), 0, st, y_branch, y_twin, scaling, gamma, mean, rstd, out, grad_out,
                       grad_loss, g, n_all, rec, g_branch, g_twin, ysum);
    hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3((unsigned)C + 1), dim3(kThreads), 0, st, rec, ysum, B, g, g_gamma, g_beta,
                       g_scaling);
    return (int)hipGetLastError();
}

}  // extern "C"
