// nms.hip -- batched box NMS as ONE launch for a batch (C ABI: zira_nms_f32, include/zira_nms.h): torchvision.ops.nms per
// image and, with labels, _batched_nms_vanilla, on the padded outputs of the detection and grounding tails and their device
// counts, with padded outputs and a count per image.  Bit-identical to nms.nms_reference.
//
// One 1024-thread block per image (K <= 1024 candidates, a batch of one or two: this is a latency kernel).  All in LDS:
//   1. thread t takes score t (nothing at and behind n[b]) through the stable descending sort of stable_desc.h; rank r then
//      holds its box, area, label and source index.  Everything below is in rank space, so "earlier" is "smaller";
//   2. the suppression relation R[i][j] = j > i && iou(i, j) > thr && label[i] == label[j] as 64-bit words: wave `i % 16`
//      builds row i, lane l of it decides j = 64 w + l for each word w >= i / 64 and the ballot IS the word.  Only the words
//      from the diagonal on are stored (row i: W - i / 64 of them, 68 KB at K = 1024 in place of 128 KB);
//   3. wave 0 sweeps the ranks, lane w holding word w of the running "removed" set.  Per group of 64 ranks: lane l fetches
//      the diagonal word of rank 64 g + l, the 64 decisions of the group are a scalar chain over v_readlane (no memory in the
//      chain), then each lane ORs its word of the kept ranks' rows -- independent LDS reads, contiguous across the lanes;
//   4. position p of `keep` is written from LDS, -1 at and behind the count.
// The diagonal fetch of 3. strides rows (up to a 16-way bank conflict, once per group of 64 ranks); every other LDS access is
// contiguous across the lanes or one address for the wave.
// No atomics, no workspace, no host synchronisation, nothing that a replayed capture could find stale.
//
// Compiled with -ffp-contract=off and the correctly rounded divide (build.EXTRA_FLAGS): the IoU is torch's fp32 arithmetic,
// every operation rounded on its own.  fminf / fmaxf differ from torch's minimum / maximum / clamp only on a NaN operand, and a
// pair that meets one (a NaN coordinate, or inf - inf) has a NaN area on one side, so a NaN union, so a NaN IoU either way.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"
#include "stable_desc.h"
#include "zira_nms.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

// words of the relation for W = ceil(K / 64) word columns: 64 rows of W - g words for g = 0 .. W - 1
constexpr size_t rel_words(int W) { return (size_t)32 * W * (W + 1); }

// where row i's diagonal word (word i / 64) stands; word w >= i / 64 of the row is w - i / 64 behind it
__device__ __forceinline__ int rel_row(int i, int W)
{
    const int g = i >> 6;
    return 64 * (g * W - g * (g - 1) / 2) + (i & 63) * (W - g);
}

// lane l's v in every lane; l is the same in every lane
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

inline size_t lds_bytes(int K)
{
    const int W = (K + 63) / 64, Kc = 64 * W;
    int P = 1;
    while (P < K) P <<= 1;
    // box 16, label 8, area 4, order 4, kept 4 per rank; the sort's exchange buffer; the relation
    return (size_t)Kc * 36 + (size_t)P * 8 + rel_words(W) * 8;
}

__global__ __launch_bounds__(kThreads) void nms_kernel(const float4 *__restrict__ boxes, const float *__restrict__ scores,
                                                       const long long *__restrict__ labels, const int32_t *__restrict__ n,
                                                       int K, int P, int W, float thr, int32_t *__restrict__ keep,
                                                       int32_t *__restrict__ n_keep)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int s_count;
    const int Kc = 64 * W;
    float4 *s_box = reinterpret_cast<float4 *>(lds);                                   // [Kc] by rank, as everything below
    unsigned long long *s_exch = reinterpret_cast<unsigned long long *>(s_box + Kc);   // [P]
    unsigned long long *s_rel = s_exch + P;                                            // [rel_words(W)]
    long long *s_label = reinterpret_cast<long long *>(s_rel + rel_words(W));          // [Kc]
    float *s_area = reinterpret_cast<float *>(s_label + Kc);                           // [Kc]
    int32_t *s_order = reinterpret_cast<int32_t *>(s_area + Kc);                       // [Kc] rank -> candidate
    int32_t *s_kept = s_order + Kc;                                                    // [Kc] output position -> rank

    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t o = (size_t)b * K;
    int m = n[b];
    m = m < 0 ? 0 : (m > K ? K : m);
    const int Wm = (m + 63) >> 6;

    // ---- 1. the visiting order (an entry of a candidate is never 0: the rows at and behind m sink behind all of them)
    unsigned long long v = t < m ? entry_of(key_of(scores[o + t]), (uint32_t)t) : 0ull;
    v = bitonic_desc(v, P, s_exch);
    if (t < m) {
        const int idx = (int)index_of(v);
        const float4 bx = boxes[o + idx];
        s_box[t] = bx;
        s_area[t] = (bx.z - bx.x) * (bx.w - bx.y);
        s_label[t] = labels ? labels[o + idx] : 0ll;
        s_order[t] = idx;
    }
    __syncthreads();

    // ---- 2. the relation, row by row
    for (int i = wave; i < m; i += kWaves) {
        const float4 bi = s_box[i];
        const float ai = s_area[i];
        const long long li = s_label[i];
        const int g = i >> 6;
        unsigned long long *row = s_rel + rel_row(i, W) - g;
        for (int w = g; w < Wm; ++w) {
            const int j = 64 * w + lane;
            bool hit = false;
            if (j > i && j < m) {
                const float4 bj = s_box[j];
                const float iw = fmaxf(0.f, fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x));
                const float ih = fmaxf(0.f, fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y));
                const float inter = iw * ih;
                const float iou = inter / (ai + s_area[j] - inter);
                hit = iou > thr && s_label[j] == li;          // strict; false for a NaN IoU
            }
            const unsigned long long word = __ballot(hit);
            if (lane == 0) row[w] = word;
        }
    }
    __syncthreads();

    // ---- 3. the sweep: one wave, lane w holds word w of the removed set
    if (wave == 0) {
        unsigned long long removed = 0ull;
        int count = 0;
        for (int g = 0; g < Wm; ++g) {
            const int i = 64 * g + lane;
            const int base = rel_row(64 * g, W), stride = W - g;
            const unsigned long long diag = i < m ? s_rel[base + lane * stride] : 0ull;
            unsigned long long cur = readlane64(removed, g);      // the same in every lane from here on
            const int live = m - 64 * g < 64 ? m - 64 * g : 64;
            for (int l = 0; l < live; ++l)
                if (!((cur >> l) & 1ull)) cur |= readlane64(diag, l);
            const unsigned long long kept = ~cur & (live == 64 ? ~0ull : (1ull << live) - 1ull);
            if ((kept >> lane) & 1ull) s_kept[count + __popcll(kept & ((1ull << lane) - 1ull))] = i;
            count += __popcll(kept);
            if (lane > g && lane < Wm) {
                unsigned long long acc = 0ull;
                for (unsigned long long r = kept; r != 0ull; r &= r - 1ull)
                    acc |= s_rel[base + (__ffsll((long long)r) - 1) * stride + (lane - g)];
                removed |= acc;
            }
        }
        if (lane == 0) s_count = count;
    }
    __syncthreads();

    // ---- 4. the kept candidates, position by position; -1 at and behind the count
    const int count = s_count;
    if (t < K) keep[o + t] = t < count ? s_order[s_kept[t]] : -1;
    if (t == 0) n_keep[b] = count;
}

inline bool served(long long B, long long K) { return B >= 1 && B <= ZIRA_NMS_MAX_B && K >= 1 && K <= ZIRA_NMS_MAX_K; }

}  // namespace

extern "C" size_t zira_nms_lds_bytes(int K)
{
    return served(1, K) ? lds_bytes(K) : 0;
}

extern "C" int zira_nms_f32(const float *boxes, const float *scores, const int64_t *labels, const int32_t *n, int B, int K,
                            float iou_threshold, int32_t *keep, int32_t *n_keep, void *stream)
{
    if (!boxes || !scores || !n || !keep || !n_keep || !served(B, K)) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)boxes & 15) || ((uintptr_t)labels & 7)) return ZIRA_MSDA_EINVAL;   // a box moves as one; (NULL labels pass)
    if (((uintptr_t)scores | (uintptr_t)n | (uintptr_t)keep | (uintptr_t)n_keep) & 3) return ZIRA_MSDA_EINVAL;
    static_assert(ZIRA_NMS_MAX_K <= kThreads, "one thread per candidate");
    const int W = (K + 63) / 64;
    int P = 1;
    while (P < K) P <<= 1;
    const size_t lds = lds_bytes(K);                    // 112 KB at K = 1024, of a CU's 160 KB
    const hipError_t e = zira::lds_opt_in(nms_kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nms_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(boxes), scores, reinterpret_cast<const long long *>(labels), n, K, P, W,
                       iou_threshold, keep, n_keep);
    return (int)hipGetLastError();
}
