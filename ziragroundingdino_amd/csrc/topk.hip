// topk.hip -- row-wise top-k as ONE launch, a pure function of the input (C ABI: zira_topk_rows_f32), and the evaluation tail
// that consumes it in the same launch (zira_detections_f32).
//
// Definition: the first k entries of a STABLE DESCENDING sort of the row -- values descending, equal values by ascending index,
// -0.0 == +0.0, NaN in front of every number (NaNs equal among themselves), as torch.sort(descending=True, stable=True).
//
// One 1024-thread block per row (the model has two rows: this is a latency kernel).
//   1. every element becomes a 32-bit key whose unsigned order is the sort's order (larger key = earlier);  a row of up to
//      kLdsMaxN elements is read once and its keys stay in LDS, a longer row is re-read (from L2) by every pass;
//   2. MSB-first radix select, 8 bits x 4 passes over LDS histograms -> the k-th largest key T and how many keys lie above it;
//   3. the keys above T and the lowest-index (k - above) keys equal to T are compacted into a candidate list: every wave walks
//      its own contiguous segment of the row, so ballots and a 16-entry scan give each tie its rank in index order;
//   4. the k candidates, as (key << 32 | ~index), are sorted descending by a bitonic network: the steps inside a wave are
//      register exchanges, the ten steps across waves go through LDS;
//   5. values are re-read through the index (the input's bit patterns, not the canonicalised key).
// No global atomics, no workspace traffic, no host synchronisation, nothing that a replayed capture could find stale.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"
#include "topk_select.h"
#include "zira_msda.h"

namespace {

constexpr int kMaxN = 1 << 20;
constexpr int kMaxRows = 65535;
constexpr int kLdsMaxN = 32768;          // 128 KB of keys beside 17 KB of static LDS, of a CU's 160 KB
constexpr size_t kWorkspace = 256;       // reserved: the kernels keep their state on chip (0 must mean "not served")

// (the selection -- keys, radix select, compaction, the sort of the survivors -- and the tail behind it: topk_select.h)
template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void topk_rows_kernel(const float *__restrict__ x, int n, int k, int P,
                                                             float *__restrict__ out_val, int64_t *__restrict__ out_idx)
{
    extern __shared__ uint32_t keys[];
    __shared__ Shared s;
    const float *row = x + (size_t)blockIdx.x * n;
    const unsigned long long v = select_sorted<IN_LDS>(row, n, k, P, s, keys);
    const int t = threadIdx.x;
    if (t < k) {
        const uint32_t idx = 0xFFFFFFFFu - (uint32_t)v;
        out_idx[(size_t)blockIdx.x * k + t] = (int64_t)idx;
        out_val[(size_t)blockIdx.x * k + t] = row[idx];
    }
}

// ---- the evaluation tail: top-k over (query x class), the selected boxes in pixels of the requested output size, clipped,
// empty ones dropped (GroundingDINO.dt_inference + structures.detector_postprocess): detections_tail of topk_select.h.
template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void detections_kernel(const float *__restrict__ prob, const float *__restrict__ boxes,
                                                              int Q, int C, int k, int P, const float *__restrict__ sizes,
                                                              float *__restrict__ scores, int64_t *__restrict__ labels,
                                                              float *__restrict__ xyxy, int32_t *__restrict__ n_keep)
{
    extern __shared__ uint32_t keys[];
    __shared__ Shared s;
    const int b = blockIdx.x, n = Q * C;
    const float *row = prob + (size_t)b * n;
    const unsigned long long v = select_sorted<IN_LDS>(row, n, k, P, s, keys);
    const int t = threadIdx.x;
    float score = 0.f;
    int64_t label = 0;
    const float *box_at = boxes;
    if (t < k) {
        const uint32_t idx = 0xFFFFFFFFu - (uint32_t)v;
        const uint32_t q = idx / (uint32_t)C;
        label = (int64_t)(idx - q * (uint32_t)C);
        score = row[idx];
        box_at = boxes + ((size_t)b * Q + q) * 4;
    }
    detections_tail(t < k, score, label, box_at, b, k, sizes, s, scores, labels, xyxy, n_keep);
}

inline bool served(long long rows, long long n, long long k)
{
    return rows >= 1 && rows <= kMaxRows && k >= 1 && k <= kMaxK && n >= k && n <= kMaxN;
}

template <typename K, typename... A>
int launch(K *kernel, int rows, int n, hipStream_t stream, A... args)
{
    const size_t lds = n <= kLdsMaxN ? (size_t)n * sizeof(uint32_t) : 0;
    const hipError_t e = zira::lds_opt_in(kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(kThreads), lds, stream, args...);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t zira_topk_rows_workspace_bytes(int rows, int n, int k)
{
    return served(rows, n, k) ? kWorkspace : 0;
}

extern "C" int zira_topk_rows_f32(const float *x, int rows, int n, int k, float *out_val, int64_t *out_idx, void *ws,
                                  size_t ws_bytes, void *stream)
{
    if (!x || !out_val || !out_idx || !served(rows, n, k) || !ws || ws_bytes < kWorkspace) return ZIRA_MSDA_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = network_size(k);
    if (n <= kLdsMaxN) return launch(topk_rows_kernel<true>, rows, n, st, x, n, k, P, out_val, out_idx);
    return launch(topk_rows_kernel<false>, rows, n, st, x, n, k, P, out_val, out_idx);
}

extern "C" int zira_detections_f32(const float *prob, const float *boxes, int B, int Q, int C, int k, const float *sizes,
                                   float *scores, int64_t *labels, float *xyxy, int32_t *n_keep, void *ws, size_t ws_bytes,
                                   void *stream)
{
    if (!prob || !boxes || !sizes || !scores || !labels || !xyxy || !n_keep || Q < 1 || C < 1) return ZIRA_MSDA_EINVAL;
    const long long n = (long long)Q * C;
    if (!served(B, n, k) || !ws || ws_bytes < kWorkspace) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)boxes | (uintptr_t)xyxy) & 15) return ZIRA_MSDA_EINVAL;   // rows of four floats move as one
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = network_size(k);
    if (n <= kLdsMaxN)
        return launch(detections_kernel<true>, B, (int)n, st, prob, boxes, Q, C, k, P, sizes, scores, labels, xyxy, n_keep);
    return launch(detections_kernel<false>, B, (int)n, st, prob, boxes, Q, C, k, P, sizes, scores, labels, xyxy, n_keep);
}
