// vocab.hip -- the merged detections tail of a chunked vocabulary as ONE launch for a batch (C ABI: zira_det_merge_f32,
// include/zira_vocab.h).  A category list longer than one caption runs as J chunks; each leaves its top-k candidates (value
// and flat index, zira_topk_rows_f32) in its slice of a candidate row, its own boxes and its own label numbering.  This kernel
// takes the first k of the stable descending order of the whole row -- which is the first k of the order of the virtual row
// cat_j(prob_j.flatten()), because an element of the global top-k has fewer than k elements before it inside its own chunk and
// chunk-major positions reproduce the tie order -- and runs the evaluation tail on them.  Bit-identical to
// vocab.detections_chunked_reference.
//
// One 1024-thread block per image (a batch of one or two: a latency kernel), built from the two pieces topk.hip is built from
// (topk_select.h):
//   1. select, then sort the survivors: the row's N <= 16384 order-preserving keys stay in LDS (64 KB), an MSB-first radix
//      select finds the k-th key, ballots compact the k survivors with the lowest-position ties, a bitonic network sorts them.
//      Sorting all N instead would be a network of 105 steps over 16 entries per thread where this is 55 steps over one entry
//      behind six passes over the keys; only the first k need an order;
//   2. thread t looks its position up in the chunk table (by value in the kernel arguments, copied to LDS once; a binary search
//      of at most six steps), reads the candidate's flat index, splits it into query and class with the chunk's C_j, and hands
//      score, global label and the address of the chunk's box to detections_tail: box to pixels of the output size, clip, drop
//      empty, compact, zero at and behind the count -- the code the detections kernel runs.
// No global atomics, no workspace, no host synchronisation, nothing that a replayed capture could find stale.
//
// The box arithmetic is spelled with the rounding intrinsics (topk_select.h) and this file is built with -ffp-contract=off
// (build.EXTRA_FLAGS), so nothing is left to the compiler's contraction default.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"
#include "topk_select.h"
#include "zira_vocab.h"

namespace {

struct ChunkTable {
    int32_t start[ZIRA_VOCAB_MAX_CHUNKS], classes[ZIRA_VOCAB_MAX_CHUNKS], label_offset[ZIRA_VOCAB_MAX_CHUNKS];
};

__global__ __launch_bounds__(kThreads) void det_merge_kernel(const float *__restrict__ cand_scores,
                                                             const long long *__restrict__ cand_index, zira_vocab_chunks c,
                                                             const float *__restrict__ boxes, int B, int Q, int k, int ksel, int P,
                                                             const float *__restrict__ sizes, float *__restrict__ scores,
                                                             int64_t *__restrict__ labels, float *__restrict__ xyxy,
                                                             int32_t *__restrict__ n_keep)
{
    extern __shared__ uint32_t keys[];
    __shared__ Shared s;
    __shared__ ChunkTable tab;
    const int b = blockIdx.x, t = threadIdx.x, N = c.n;
    if (t < c.J) {   // (read behind the barriers of the selection)
        tab.start[t] = c.start[t];
        tab.classes[t] = c.classes[t];
        tab.label_offset[t] = c.label_offset[t];
    }
    const float *row = cand_scores + (size_t)b * N;
    const unsigned long long v = select_sorted<true>(row, N, ksel, P, s, keys);

    float score = 0.f;
    int64_t label = 0;
    const float *box_at = boxes;
    if (t < ksel) {
        const int p = (int)index_of(v);
        int lo = 0, hi = c.J - 1;                     // the last chunk whose start is not behind p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab.start[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const uint32_t C = (uint32_t)tab.classes[lo], QC = (uint32_t)Q * C;      // (Q * C_j < 2^31: checked on the host)
        const long long flat = cand_index[(size_t)b * N + p];
        const uint32_t f = flat < 0 || flat >= (long long)QC ? QC - 1u : (uint32_t)flat;   // never a read outside `boxes`
        const uint32_t q = f / C;
        label = (int64_t)tab.label_offset[lo] + (int64_t)(f - q * C);
        score = row[p];
        box_at = boxes + (((size_t)lo * B + b) * Q + q) * 4;
    }
    detections_tail(t < ksel, score, label, box_at, b, k, sizes, s, scores, labels, xyxy, n_keep);
}

inline bool served(long long B, long long n, long long k)
{
    return B >= 1 && B <= ZIRA_VOCAB_MAX_B && n >= 1 && n <= ZIRA_VOCAB_MAX_CANDIDATES && k >= 1 && k <= ZIRA_VOCAB_MAX_K;
}

inline bool table_ok(const zira_vocab_chunks &c, int Q)
{
    if (c.J < 1 || c.J > ZIRA_VOCAB_MAX_CHUNKS || c.start[0] != 0) return false;
    for (int j = 0; j < c.J; ++j) {
        const long long end = j + 1 < c.J ? c.start[j + 1] : c.n;
        if (c.start[j] < 0 || end <= c.start[j]) return false;                     // strictly ascending, below n
        if (c.classes[j] < 1 || c.label_offset[j] < 0) return false;
        if ((long long)Q * c.classes[j] > INT32_MAX || (long long)c.label_offset[j] + c.classes[j] > INT32_MAX) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t zira_det_merge_lds_bytes(int n)
{
    // the keys (dynamic), the selection's state and the chunk table (static)
    return served(1, n, 1) ? (size_t)n * sizeof(uint32_t) + sizeof(Shared) + sizeof(ChunkTable) : 0;
}

extern "C" int zira_det_merge_f32(const float *cand_scores, const int64_t *cand_index, const zira_vocab_chunks *chunks,
                                  const float *boxes, int B, int Q, int k, const float *sizes, float *scores, int64_t *labels,
                                  float *xyxy, int32_t *n_keep, void *stream)
{
    static_assert(ZIRA_VOCAB_MAX_K <= kMaxK && ZIRA_VOCAB_MAX_K <= kThreads, "one thread per output row");
    static_assert((size_t)ZIRA_VOCAB_MAX_CANDIDATES * 4 + sizeof(Shared) + sizeof(ChunkTable) <= 160 * 1024, "a CU's LDS");
    if (!cand_scores || !cand_index || !chunks || !boxes || !sizes || !scores || !labels || !xyxy || !n_keep) return ZIRA_MSDA_EINVAL;
    if (Q < 1 || !served(B, chunks->n, k) || !table_ok(*chunks, Q)) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)boxes | (uintptr_t)xyxy) & 15) return ZIRA_MSDA_EINVAL;            // rows of four floats move as one
    if (((uintptr_t)cand_index | (uintptr_t)labels) & 7) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)cand_scores | (uintptr_t)sizes | (uintptr_t)scores | (uintptr_t)n_keep) & 3) return ZIRA_MSDA_EINVAL;
    const zira_vocab_chunks c = *chunks;
    const int ksel = k < c.n ? k : c.n;               // k beyond the candidates: all of them, the rest of the row is zero
    const size_t lds = (size_t)c.n * sizeof(uint32_t);
    const hipError_t e = zira::lds_opt_in(det_merge_kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(det_merge_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), cand_scores,
                       reinterpret_cast<const long long *>(cand_index), c, boxes, B, Q, k, ksel, network_size(ksel), sizes, scores,
                       labels, xyxy, n_keep);
    return (int)hipGetLastError();
}
