// metrics.hip -- the training metrics log on the device (C ABI: zira_metrics_record_f32, zira_metrics_window_f64; contract in
// include/zira_metrics.h).
//
// record: one wave; lane c copies the bits of column c of this iteration (a device scalar or a host value from the kernel's
// arguments) into the ring's row `cursor % rows`, a ballot over the loss columns' exponent fields finds an inf / NaN, lane 0
// sets first_bad where it is still -1 and then advances the cursor.  The cursor lives on the device, so the launch carries no
// per-iteration host value besides the host columns and can be captured.
//
// window: one wave per output column (the cols columns, then total_loss); lane i holds row i of the window, oldest first.
// Every lane computes its row's value over the ranks in numpy's order; the wave then ranks the values by counting (64
// lane reads), picks the middle one or two by ballot, and every lane runs numpy's pairwise sum over the lane values for the
// mean.  fp64 throughout, no contraction: the bits are numpy's.  No LDS, no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "zira_metrics.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMaxRanks = ZIRA_METRICS_MAX_RANKS;
static_assert(ZIRA_METRICS_MAX_COLS <= kWave && ZIRA_METRICS_MAX_WINDOW <= kWave, "one lane per column, one lane per window row");
static_assert(kMaxRanks == 8, "rank_value spells numpy's pairwise sum for at most 8 values");

__global__ __launch_bounds__(kWave) void record_kernel(zira_metrics_sources s, float *__restrict__ ring, int rows,
                                                       int64_t *__restrict__ cursor, int64_t *__restrict__ first_bad)
{
    const int c = threadIdx.x;
    const int cols = s.n_dev + s.n_host;
    const long long cur = *cursor;
    const long long bad = *first_bad;
    uint32_t bits = 0;
    if (c < s.n_dev)
        bits = *reinterpret_cast<const uint32_t *>(s.src[c]);
    else if (c < cols)
        bits = __float_as_uint(s.host[c - s.n_dev]);
    long long row = cur % rows;
    if (row < 0) row += rows;      // a cursor the caller never initialised: stay inside the ring
    if (c < cols) reinterpret_cast<uint32_t *>(ring)[row * cols + c] = bits;
    const bool non_finite = c < s.n_loss && (bits & 0x7f800000u) == 0x7f800000u;
    const bool any = __ballot(non_finite) != 0;
    if (c == 0) {
        if (bad == -1 && any) *first_bad = cur;
        *cursor = cur + 1;
    }
}

// One column of one row over the ranks: np.mean of a list of `ranks` values (np.max where use_max).
__device__ __forceinline__ double rank_value(const float *__restrict__ p, long long stride, int ranks, bool use_max)
{
    double v[kMaxRanks];
#pragma unroll
    for (int r = 0; r < kMaxRanks; ++r) v[r] = r < ranks ? (double)p[r * stride] : 0.0;
    if (use_max) {
        double m = v[0];
#pragma unroll
        for (int r = 1; r < kMaxRanks; ++r)
            if (r < ranks && m == m && (v[r] != v[r] || v[r] > m)) m = v[r];
        return m;
    }
    double sum;
    if (ranks < 8) {
        sum = -0.0;
#pragma unroll
        for (int r = 0; r < kMaxRanks - 1; ++r)
            if (r < ranks) sum = sum + v[r];
    } else {
        sum = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    return (0.0 + sum) / (double)ranks;
}

__global__ __launch_bounds__(kWave) void window_kernel(const float *__restrict__ rings, long long rank_stride, int ranks, int rows,
                                                       int cols, const int64_t *__restrict__ cursor, int window, int n_loss,
                                                       int max_col, double *__restrict__ out)
{
    const int c = blockIdx.x;      // cols: total_loss
    const int lane = threadIdx.x;
    const int ld = cols + 1;
    const long long cur = *cursor;
    const int n = (int)(cur < window ? cur : window);      // wave-uniform
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (n <= 0) {
        if (lane < 3) out[lane * ld + c] = nan;
        return;
    }
    double v = 0.0;
    if (lane < n) {
        const long long t = cur - n + lane;
        const float *row = rings + (t % rows) * cols;
        if (c < cols) {
            v = rank_value(row + c, rank_stride, ranks, c == max_col);
        } else {
            for (int k = 0; k < n_loss; ++k) v = v + rank_value(row + k, rank_stride, ranks, false);
        }
    }
    const bool any_nan = __ballot(lane < n && v != v) != 0;
    // position of this lane's value among the n: the count of smaller ones, ties in lane order
    int pos = 0;
    for (int j = 0; j < n; ++j) {
        const double u = __shfl(v, j);
        pos += (u < v || (u == v && j < lane)) ? 1 : 0;
    }
    double median = nan;
    if (!any_nan) {       // then the positions are a permutation of 0 .. n-1
        const int k0 = (n - 1) >> 1, k1 = n >> 1;
        const unsigned long long m0 = __ballot(lane < n && pos == k0), m1 = __ballot(lane < n && pos == k1);
        const double a = __shfl(v, __ffsll(m0) - 1), b = __shfl(v, __ffsll(m1) - 1);
        median = k0 == k1 ? 0.0 + a : (0.0 + (a + b)) / 2.0;
    }
    // numpy's pairwise sum of n <= 64 doubles (every lane computes it)
    double sum;
    if (n < 8) {
        sum = -0.0;
        for (int j = 0; j < n; ++j) sum = sum + __shfl(v, j);
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = __shfl(v, j);
        int i = 8;
        for (; i < n - (n & 7); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + __shfl(v, i + j);
        }
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) sum = sum + __shfl(v, i);
    }
    const double mean = (0.0 + sum) / (double)n;
    const double latest = __shfl(v, n - 1);
    if (lane == 0) {
        out[c] = latest;
        out[ld + c] = median;
        out[2 * ld + c] = mean;
    }
}

bool aligned(const void *p, uintptr_t a) { return p != nullptr && ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int zira_metrics_record_f32(const zira_metrics_sources *sources, float *ring, int rows, int64_t *cursor,
                                       int64_t *first_bad, void *stream)
{
    if (!sources || !aligned(ring, 4) || !aligned(cursor, 8) || !aligned(first_bad, 8)) return ZIRA_MSDA_EINVAL;
    if (rows < 1 || rows > ZIRA_METRICS_MAX_ROWS) return ZIRA_MSDA_EINVAL;
    const zira_metrics_sources s = *sources;
    if (s.n_dev < 0 || s.n_dev > ZIRA_METRICS_MAX_COLS || s.n_host < 0 || s.n_host > ZIRA_METRICS_MAX_HOST) return ZIRA_MSDA_EINVAL;
    const int cols = s.n_dev + s.n_host;
    if (cols < 1 || cols > ZIRA_METRICS_MAX_COLS || s.n_loss < 0 || s.n_loss > cols) return ZIRA_MSDA_EINVAL;
    for (int i = 0; i < s.n_dev; ++i)
        if (!aligned(s.src[i], 4)) return ZIRA_MSDA_EINVAL;
    hipLaunchKernelGGL(record_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), s, ring, rows, cursor, first_bad);
    return (int)hipGetLastError();
}

extern "C" int zira_metrics_window_f64(const float *rings, int64_t rank_stride, int ranks, int rows, int cols,
                                       const int64_t *cursor, int window, int n_loss, int max_col, double *out, void *stream)
{
    if (!aligned(rings, 4) || !aligned(cursor, 8) || !aligned(out, 8)) return ZIRA_MSDA_EINVAL;
    if (ranks < 1 || ranks > ZIRA_METRICS_MAX_RANKS || rows < 1 || rows > ZIRA_METRICS_MAX_ROWS) return ZIRA_MSDA_EINVAL;
    if (cols < 1 || cols > ZIRA_METRICS_MAX_COLS || window < 1 || window > ZIRA_METRICS_MAX_WINDOW || window > rows)
        return ZIRA_MSDA_EINVAL;
    if (n_loss < 0 || n_loss > cols || !(max_col == -1 || (max_col >= n_loss && max_col < cols))) return ZIRA_MSDA_EINVAL;
    if (ranks > 1 && rank_stride < (int64_t)rows * cols) return ZIRA_MSDA_EINVAL;
    hipLaunchKernelGGL(window_kernel, dim3(cols + 1), dim3(kWave), 0, static_cast<hipStream_t>(stream), rings,
                       (long long)(ranks > 1 ? rank_stride : 0), ranks, rows, cols, cursor, window, n_loss, max_col, out);
    return (int)hipGetLastError();
}
