// prompt_memory.hip -- the text-memory replay's loss, L1Loss(mean) between the encoded text and itself with the learned
// categories' rows replaced by their pool entries, forward and backward, ONE launch each (C ABI: zira_pmem_supported,
// zira_pmem_workspace_bytes, zira_pmem_loss_{fwd,bwd}_f32; contract in include/zira_prompt_memory.h).  The index tables are
// prompt.hip's, unchanged.
//
// A few hundred KB are read once: what counts is the launch count and that nothing is read back to the host.  One wave owns one
// row of D floats and reads it as 16-byte vectors, a quarter row per lane and round.
//   forward:  wave i < B * T takes |pool - x| of row i where the table names a pool row (fp32 difference and absolute value, as
//             ATen's), adds in double, the block's four waves are added in wave order and thread 0 writes the block's double to
//             the workspace, releases it and draws an integer ticket; the block that draws the last one acquires, adds the
//             blocks' doubles in index order with plain loads and stores (float)(S / N).  The ticket wraps to zero on the last
//             draw (atomicInc), so the next call -- or a graph replay -- finds it as the first one did.
//   backward: with g_pool asked for, wave i < n_rows sums +sign(pool - x) * s over pool row i's occurrence list, in list order,
//             in registers, and stores the row once (zeros for an empty list); with gx asked for, the next B * T waves write
//             -sign(pool - x) * s or zeros.  s = g * (1 / N), g read from the device.  No atomics, no LDS, no workspace.
// Every index read from a table is checked against its buffer before it is used.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "prompt_table.h"
#include "ticket.h"
#include "zero_loss.h"
#include "zira_prompt.h"
#include "zira_prompt_memory.h"

namespace {

using namespace prompt_table;      // kThreads, kWave, kWavesPerBlock, f4, pool_row_of, aligned*, blocks_of
constexpr size_t kTicketBytes = 16;      // the workspace's head: the ticket word, padded so that the doubles stay aligned

__global__ __launch_bounds__(kThreads) void pmem_fwd_kernel(const float *__restrict__ x, const int32_t *__restrict__ table,
                                                            const zira_prompt_segment *__restrict__ segments, int n_pos, int D,
                                                            int n_segments, double inv_n, float *__restrict__ loss,
                                                            unsigned *__restrict__ ticket, double *__restrict__ part)
{
    __shared__ double wave_sum[kWavesPerBlock];
    __shared__ int is_last;
    const int wave = (int)(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const int pos = blockIdx.x * kWavesPerBlock + wave;
    double acc = 0.0;
    if (pos < n_pos) {
        const float *p = pool_row_of(table, segments, pos, D, n_segments);
        if (p != nullptr) {
            const float *src = x + (size_t)pos * D;
            for (int v = lane; v < D / 4; v += kWave) {
                const f4 a = *reinterpret_cast<const f4 *>(p + 4 * v), b = *reinterpret_cast<const f4 *>(src + 4 * v);
                const f4 d = a - b;
                acc += (double)__builtin_fabsf(d.x);
                acc += (double)__builtin_fabsf(d.y);
                acc += (double)__builtin_fabsf(d.z);
                acc += (double)__builtin_fabsf(d.w);
            }
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);      // (lane_sum.h's lane_sum_xor64, inline)
    if (lane == 0) wave_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) s += wave_sum[w];
        part[blockIdx.x] = s;
        release_agent();
        is_last = atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1;      // wraps to 0 behind the last block: ready for the next call
    }
    __syncthreads();
    if (!is_last || threadIdx.x != 0) return;
    acquire_agent();
    // (behind the acquire fence plain loads see the other blocks' doubles, and unlike atomic loads they are issued ahead of
    //  their use)
    double total = 0.0;
#pragma unroll 8
    for (unsigned i = 0; i < gridDim.x; ++i) total += part[i];
    *loss = (float)(total * inv_n);
}

__global__ __launch_bounds__(kThreads) void pmem_bwd_kernel(const float *__restrict__ grad_loss, const float *__restrict__ x,
                                                            const int32_t *__restrict__ table,
                                                            const zira_prompt_segment *__restrict__ segments,
                                                            const int32_t *__restrict__ occ_start, const int32_t *__restrict__ occ,
                                                            int n_pos, int D, int n_segments, int n_rows, int n_occ, float inv_n,
                                                            float *__restrict__ g_pool, float *__restrict__ gx)
{
    const int unit = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    const float s = grad_loss[0] * inv_n;
    if (unit < n_rows) {
        int lo = occ_start[unit], hi = occ_start[unit + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_occ ? n_occ : hi;
        float *dst = g_pool + (size_t)unit * D;
        for (int v = lane; v < D / 4; v += kWave) {
            f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = lo; k < hi; ++k) {
                const int pos = occ[k];
                if (pos < 0 || pos >= n_pos) continue;
                const float *p = pool_row_of(table, segments, pos, D, n_segments);
                if (p == nullptr) continue;
                const f4 d = *reinterpret_cast<const f4 *>(p + 4 * v) - *reinterpret_cast<const f4 *>(x + (size_t)pos * D + 4 * v);
                acc.x += sign_of(d.x) * s;
                acc.y += sign_of(d.y) * s;
                acc.z += sign_of(d.z) * s;
                acc.w += sign_of(d.w) * s;
            }
            *reinterpret_cast<f4 *>(dst + 4 * v) = acc;
        }
        return;
    }
    const int pos = unit - n_rows;
    if (gx == nullptr || pos >= n_pos) return;
    const float *p = pool_row_of(table, segments, pos, D, n_segments);
    const float *src = x + (size_t)pos * D;
    float *dst = gx + (size_t)pos * D;
    for (int v = lane; v < D / 4; v += kWave) {
        f4 val = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p != nullptr) {
            const f4 d = *reinterpret_cast<const f4 *>(p + 4 * v) - *reinterpret_cast<const f4 *>(src + 4 * v);
            val.x = -(sign_of(d.x) * s);
            val.y = -(sign_of(d.y) * s);
            val.z = -(sign_of(d.z) * s);
            val.w = -(sign_of(d.w) * s);
        }
        *reinterpret_cast<f4 *>(dst + 4 * v) = val;
    }
}

}  // namespace

extern "C" int zira_pmem_supported(int B, int T, int D, int n_segments, long long n_rows)
{
    return zira_prompt_supported(B, T, D, n_segments, n_rows);
}

extern "C" size_t zira_pmem_workspace_bytes(int B, int T)
{
    if (B < 1 || B > ZIRA_PROMPT_MAX_B || T < 1 || T > ZIRA_PROMPT_MAX_T) return 0;
    return kTicketBytes + sizeof(double) * (size_t)blocks_of((long long)B * T);
}

extern "C" int zira_pmem_loss_fwd_f32(const float *x, const int32_t *table, const void *segments, int B, int T, int D, int n_segments,
                                      float *loss, void *workspace, void *stream)
{
    if (!zira_pmem_supported(B, T, D, n_segments, 1)) return -1;
    if (!aligned16(x) || !aligned4(table) || !aligned8(segments) || !aligned4(loss) || !aligned16(workspace)) return -1;
    const int n_pos = B * T;
    const double inv_n = 1.0 / ((double)n_pos * (double)D);
    hipLaunchKernelGGL(pmem_fwd_kernel, dim3(blocks_of(n_pos)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, table,
                       static_cast<const zira_prompt_segment *>(segments), n_pos, D, n_segments, inv_n, loss,
                       static_cast<unsigned *>(workspace),
                       reinterpret_cast<double *>(static_cast<char *>(workspace) + kTicketBytes));
    return (int)hipGetLastError();
}

extern "C" int zira_pmem_loss_bwd_f32(const float *grad_loss, const float *x, const int32_t *table, const void *segments,
                                      const int32_t *occ_start, const int32_t *occ, int B, int T, int D, int n_segments,
                                      long long n_rows, int n_occ, float *g_pool, float *gx, void *stream)
{
    if (!zira_pmem_supported(B, T, D, n_segments, n_rows)) return -1;
    if (n_occ < 0 || n_occ > B * T) return -1;
    if (!aligned4(grad_loss) || !aligned16(x) || !aligned4(table) || !aligned8(segments)) return -1;
    if (g_pool != nullptr && (!aligned16(g_pool) || !aligned4(occ_start) || !aligned4(occ))) return -1;
    if (gx != nullptr && !aligned16(gx)) return -1;
    if (g_pool == nullptr && gx == nullptr) return 0;
    const int n_pos = B * T;
    const int pool_units = g_pool != nullptr ? (int)n_rows : 0;
    const long long units = (long long)pool_units + (gx != nullptr ? n_pos : 0);
    // ATen's mean backward divides by a host scalar: on the device that is a product with the fp32 reciprocal
    const float inv_n = 1.0f / (float)((long long)n_pos * D);
    hipLaunchKernelGGL(pmem_bwd_kernel, dim3(blocks_of(units)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), grad_loss, x,
                       table, static_cast<const zira_prompt_segment *>(segments), occ_start, occ, n_pos, D, n_segments, pool_units,
                       n_occ, inv_n, g_pool, gx);
    return (int)hipGetLastError();
}
