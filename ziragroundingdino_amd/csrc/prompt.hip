// prompt.hip -- the prompt-tuning baseline's substitution of pool entries into the encoded text, forward and backward, ONE
// launch each (C ABI: zira_prompt_supported, zira_prompt_substitute_{fwd,bwd}_f32; contract in include/zira_prompt.h).
//
// A gather and its transpose over a few hundred KB: what counts is the launch count and that nothing is read back to the
// host.  One wave owns one row of D floats and moves it as 16-byte vectors, a quarter row per lane and round.
//   forward:  wave i < B * T writes out row i from x or from the pool entry the table names (reached through the segment table).
//   backward: wave i < n_rows sums the rows of grad_out on pool row i's occurrence list, in list order, in registers, and
//             stores the row once (zeros for an empty list); with gx asked for, wave n_rows + j writes gx row j (grad_out's row
//             or zeros).  No atomics, no LDS, no workspace.
// Every index read from a table is checked against its buffer before it is used.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "zira_prompt.h"
#include "prompt_table.h"

namespace {

using namespace prompt_table;      // kThreads, kWave, kWavesPerBlock, f4, pool_row_of, aligned*, blocks_of

__global__ __launch_bounds__(kThreads) void prompt_fwd_kernel(const float *__restrict__ x, const int32_t *__restrict__ table,
                                                              const zira_prompt_segment *__restrict__ segments, int n_pos, int D,
                                                              int n_segments, float *__restrict__ out)
{
    const int pos = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    if (pos >= n_pos) return;
    const int lane = threadIdx.x % kWave;
    const float *row = pool_row_of(table, segments, pos, D, n_segments);
    const float *src = row != nullptr ? row : x + (size_t)pos * D;
    float *dst = out + (size_t)pos * D;
    for (int v = lane; v < D / 4; v += kWave)
        *reinterpret_cast<f4 *>(dst + 4 * v) = *reinterpret_cast<const f4 *>(src + 4 * v);
}

__global__ __launch_bounds__(kThreads) void prompt_bwd_kernel(const float *__restrict__ g, const int32_t *__restrict__ table,
                                                              const int32_t *__restrict__ occ_start,
                                                              const int32_t *__restrict__ occ, int n_pos, int D, int n_rows,
                                                              int n_occ, float *__restrict__ g_pool, float *__restrict__ gx)
{
    const int unit = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    if (unit < n_rows) {
        int lo = occ_start[unit], hi = occ_start[unit + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_occ ? n_occ : hi;
        float *dst = g_pool + (size_t)unit * D;
        for (int v = lane; v < D / 4; v += kWave) {
            f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = lo; k < hi; ++k) {
                const int pos = occ[k];
                if (pos >= 0 && pos < n_pos) acc += *reinterpret_cast<const f4 *>(g + (size_t)pos * D + 4 * v);
            }
            *reinterpret_cast<f4 *>(dst + 4 * v) = acc;
        }
        return;
    }
    const int pos = unit - n_rows;
    if (gx == nullptr || pos >= n_pos) return;
    const bool kept = table[2 * pos] < 0;
    const float *src = g + (size_t)pos * D;
    float *dst = gx + (size_t)pos * D;
    for (int v = lane; v < D / 4; v += kWave) {
        f4 val = {0.0f, 0.0f, 0.0f, 0.0f};
        if (kept) val = *reinterpret_cast<const f4 *>(src + 4 * v);
        *reinterpret_cast<f4 *>(dst + 4 * v) = val;
    }
}

}  // namespace

extern "C" int zira_prompt_supported(int B, int T, int D, int n_segments, long long n_rows)
{
    return B >= 1 && B <= ZIRA_PROMPT_MAX_B && T >= 1 && T <= ZIRA_PROMPT_MAX_T && D >= 4 && D <= ZIRA_PROMPT_MAX_D && D % 4 == 0
           && n_segments >= 1 && n_segments <= ZIRA_PROMPT_MAX_SEGMENTS && n_rows >= 1 && n_rows <= ZIRA_PROMPT_MAX_ROWS;
}

extern "C" int zira_prompt_substitute_fwd_f32(const float *x, const int32_t *table, const zira_prompt_segment *segments, int B,
                                              int T, int D, int n_segments, float *out, void *stream)
{
    if (!zira_prompt_supported(B, T, D, n_segments, 1)) return -1;
    if (!aligned16(x) || !aligned16(out) || !aligned4(table) || !aligned8(segments)) return -1;
    const int n_pos = B * T;
    hipLaunchKernelGGL(prompt_fwd_kernel, dim3(blocks_of(n_pos)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, table, segments,
                       n_pos, D, n_segments, out);
    return (int)hipGetLastError();
}

extern "C" int zira_prompt_substitute_bwd_f32(const float *grad_out, const int32_t *table, const int32_t *occ_start,
                                              const int32_t *occ, int B, int T, int D, long long n_rows, int n_occ, float *g_pool,
                                              float *gx, void *stream)
{
    if (!zira_prompt_supported(B, T, D, 1, n_rows)) return -1;
    if (n_occ < 0 || n_occ > B * T) return -1;
    if (!aligned16(grad_out) || !aligned16(g_pool) || !aligned4(table) || !aligned4(occ_start) || !aligned4(occ)) return -1;
    if (gx != nullptr && !aligned16(gx)) return -1;
    const int n_pos = B * T;
    const long long units = n_rows + (gx != nullptr ? n_pos : 0);
    hipLaunchKernelGGL(prompt_bwd_kernel, dim3(blocks_of(units)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad_out, table,
                       occ_start, occ, n_pos, D, (int)n_rows, n_occ, g_pool, gx);
    return (int)hipGetLastError();
}
