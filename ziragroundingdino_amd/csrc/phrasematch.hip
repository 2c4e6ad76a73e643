// phrasematch.hip -- phrase-grounding matching for a whole batch as ONE launch (C ABI: zira_phrase_match_f32): per (image,
// phrase) the phrase's score of every query, the first k_max queries of the stable descending order, their boxes in the frame
// of the ground truth, the best fp64 IoU of each with the phrase's GT boxes and the rank of the first hit per threshold -- what
// Recall@k and Precision@IoU are counted from (phrase_evaluation.py).  The rules are stated in include/zira_phrase.h.
//
// One workgroup per (image, phrase), as many threads as the sorting network over the Q scores has entries (64 ... 1024):
//   0. a phrase without a token below T or without a GT box writes its padding and returns; otherwise the mask words (cut at T)
//      go to LDS and wave 0 stages the GT boxes, one lane each -- with `merged` their union box, a wave fminf / fmaxf;
//   1. the waves walk the queries, eight at a time: a group of 8 lanes forms one query's masked maximum, each lane over every
//      eighth float4 of the row (16-byte loads; a float4 whose four mask bits are clear is not loaded -- a phrase is a few of up
//      to 256 tokens), on the integer keys of stable_desc.h, so that a NaN is the largest value and -0.0 is 0.0 without a
//      float comparison; three lane exchanges, and the score goes to LDS as a float.  Rows that are not 16-byte aligned (T % 4
//      != 0) take the same walk token by token;
//   2. thread q holds the entry of query q and the block sorts them (bitonic_desc); thread r < min(k_max, Q) then holds rank r;
//   3. wave 0: candidate r belongs to the lanes r, r + R, r + 2 R ... (R the power of two at or above the candidate count);
//      each converts the box (box_to_output, the detections tail's arithmetic), walks its share of the GTs in fp64 and keeps
//      the best IoU; a wave maximum over the lanes of a candidate; a ballot per threshold finds the first hit.
// No global atomics, no workspace, no allocation, no host synchronisation: the result depends on the inputs alone.
// Contraction is off for the whole file (and on the compile line): `da + ga - w * h` stays an add, a multiply and a subtract.
//
// Bound: launch latency; a block reads at most Q rows of 1 KB (usually Q x 16 bytes) and writes a few hundred bytes.  A first
// version: nothing is tuned beyond "one launch, no sync".
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "topk_select.h"
#include "zira_phrase.h"

#pragma clang fp contract(off)

namespace {

struct PhraseArgs {
    const float *prob, *boxes, *sizes;
    const uint32_t *bits;
    const float *gt;
    const int32_t *gt_count;
    int32_t *top_query;
    float *top_score;
    double *top_iou;
    int32_t *first_hit;
    unsigned char *valid;
    double thr[ZIRA_PHRASE_MAX_THRS];
    int Q, T, P, G, k_max, n_thr, merged;
    int net;   // entries of the sorting network: the power of two at or above Q
    int R;     // the power of two at or above min(k_max, Q)
    int vec;   // the rows of prob are 16-byte aligned
};

// dynamic LDS: float4 gbox[G] | u64 exch[net] | float score[Q] | int32 cand[k_max] | uint32 mask[ceil(T / 32)]
inline size_t lds_bytes(int Q, int T, int G, int k_max)
{
    return (size_t)G * 16 + (size_t)network_size(Q) * 8 + (size_t)Q * 4 + (size_t)k_max * 4 + (size_t)((T + 31) / 32) * 4;
}

inline bool served(int Q, int T, int G, int k_max, int n_thr)
{
    return Q >= 1 && Q <= ZIRA_PHRASE_MAX_Q && T >= 1 && T <= ZIRA_PHRASE_MAX_T && G >= 1 && G <= ZIRA_PHRASE_MAX_G && k_max >= 1 &&
           k_max <= ZIRA_PHRASE_MAX_K && n_thr >= 1 && n_thr <= ZIRA_PHRASE_MAX_THRS;
}

// the float of a key of key_of: NaN as the canonical quiet NaN, the one zero as +0.0
__device__ __forceinline__ float value_of(uint32_t key)
{
    if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(1024) void phrase_match_kernel(const PhraseArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int Q = a.Q, T = a.T, G = a.G, K = a.k_max, W = (T + 31) >> 5, kc = min(K, Q);
    const long long bp = blockIdx.x;
    const int b = (int)(bp / a.P);

    float4 *gbox = reinterpret_cast<float4 *>(smem);
    unsigned long long *exch = reinterpret_cast<unsigned long long *>(gbox + G);
    float *score = reinterpret_cast<float *>(exch + a.net);
    int32_t *cand = reinterpret_cast<int32_t *>(score + Q);
    uint32_t *mask = reinterpret_cast<uint32_t *>(cand + K);

    int32_t *top_query = a.top_query + bp * K, *first_hit = a.first_hit + bp * a.n_thr;
    float *top_score = a.top_score + bp * K;
    double *top_iou = a.top_iou + bp * K;

    // ---- 0. is the phrase scored?  (the same answer in every thread)
    const uint32_t *bits = a.bits + bp * W;
    const uint32_t last = (T & 31) ? (1u << (T & 31)) - 1u : 0xFFFFFFFFu;   // bits at and above T are never looked at
    uint32_t any = 0u;
    for (int w = 0; w < W; ++w) any |= bits[w] & (w == W - 1 ? last : 0xFFFFFFFFu);
    const int gc = min(max(a.gt_count[bp], 0), G);
    if (any == 0u || gc == 0) {
        if (tid < K) top_query[tid] = -1, top_score[tid] = 0.f, top_iou[tid] = 0.0;
        if (tid < a.n_thr) first_hit[tid] = K;
        if (tid == 0) a.valid[bp] = 0;
        return;
    }
    if (tid < W) mask[tid] = bits[tid] & (tid == W - 1 ? last : 0xFFFFFFFFu);
    if (wave == 0) {   // G <= 64: one lane per GT box; the lanes behind the count hold a copy of the first
        const float *p = a.gt + (bp * G + (lane < gc ? lane : 0)) * 4;
        float4 g = make_float4(p[0], p[1], p[2], p[3]);
        if (a.merged) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                g.x = fminf(g.x, __shfl_xor(g.x, o));
                g.y = fminf(g.y, __shfl_xor(g.y, o));
                g.z = fmaxf(g.z, __shfl_xor(g.z, o));
                g.w = fmaxf(g.w, __shfl_xor(g.w, o));
            }
            if (lane == 0) gbox[0] = g;
        } else if (lane < gc) {
            gbox[lane] = g;
        }
    }
    const int ng = a.merged ? 1 : gc;
    __syncthreads();

    // ---- 1. the scores: eight queries per wave and step, eight lanes per query
    const float *prob = a.prob + (long long)b * Q * T;
    const int part = lane & 7, sub = lane >> 3;
    for (int base = wave * 8; base < Q; base += nwaves * 8) {
        const int q = base + sub;
        uint32_t key = 0u;   // below every key
        if (q < Q) {
            const float *row = prob + (long long)q * T;
            if (a.vec) {
                for (int c = part; c < (T >> 2); c += 8) {
                    const uint32_t nib = (mask[c >> 3] >> ((c & 7) * 4)) & 0xFu;
                    if (nib == 0u) continue;
                    const float4 v = *reinterpret_cast<const float4 *>(row + 4 * c);
                    if (nib & 1u) key = max(key, key_of(v.x));
                    if (nib & 2u) key = max(key, key_of(v.y));
                    if (nib & 4u) key = max(key, key_of(v.z));
                    if (nib & 8u) key = max(key, key_of(v.w));
                }
            } else {
                for (int t = part; t < T; t += 8)
                    if ((mask[t >> 5] >> (t & 31)) & 1u) key = max(key, key_of(row[t]));
            }
        }
        key = max(key, (uint32_t)__shfl_xor((int)key, 1));
        key = max(key, (uint32_t)__shfl_xor((int)key, 2));
        key = max(key, (uint32_t)__shfl_xor((int)key, 4));
        if (part == 0 && q < Q) score[q] = value_of(key);
    }
    __syncthreads();

    // ---- 2. the stable descending order; thread r holds rank r
    const unsigned long long mine = tid < Q ? entry_of(key_of(score[tid]), (uint32_t)tid) : 0ull;
    const unsigned long long entry = bitonic_desc(mine, a.net, exch);
    if (tid < kc) {
        const int q = (int)index_of(entry);
        cand[tid] = q;
        top_query[tid] = q, top_score[tid] = score[q];
    } else if (tid < K) {
        top_query[tid] = -1, top_score[tid] = 0.f, top_iou[tid] = 0.0;
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- 3. boxes, IoU and the first hit: candidate r on the lanes r, r + R, ...
    const int R = a.R, r = lane & (R - 1), first = lane / R, step = 64 / R;
    double best = 0.0;
    if (r < kc) {
        const float img_h = a.sizes[b * 2 + 0], img_w = a.sizes[b * 2 + 1];
        const float *p = a.boxes + ((long long)b * Q + cand[r]) * 4;
        const float4 px = box_to_output(make_float4(p[0], p[1], p[2], p[3]), img_h, img_w, 1.f, 1.f, img_h, img_w);
        const double x0 = px.x, y0 = px.y, x1 = px.z, y1 = px.w;
        const double da = (x1 - x0) * (y1 - y0);
        for (int g = first; g < ng; g += step) {
            const float4 gb = gbox[g];
            const double gx0 = gb.x, gy0 = gb.y, gx1 = gb.z, gy1 = gb.w;
            const double ga = (gx1 - gx0) * (gy1 - gy0);
            const double w = fmin(x1, gx1) - fmax(x0, gx0), h = fmin(y1, gy1) - fmax(y0, gy0);
            if (w > 0.0 && h > 0.0) {
                const double i = w * h;
                const double u = da + ga - i;
                const double iou = i / u;
                if (iou > best) best = iou;   // (a NaN quotient counts as 0)
            }
        }
    }
    for (int o = R; o < 64; o <<= 1) {
        const double y = __shfl_xor(best, o);
        best = y > best ? y : best;
    }
    if (lane < kc) top_iou[lane] = best;
    for (int t = 0; t < a.n_thr; ++t) {
        const unsigned long long hits = __ballot(lane < kc && best >= a.thr[t]);
        if (lane == 0) first_hit[t] = hits ? __ffsll((long long)hits) - 1 : K;
    }
    if (lane == 0) a.valid[bp] = 1;
}

inline int pow2_at_least(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" size_t zira_phrase_match_lds_bytes(int Q, int T, int G, int k_max, int n_thr)
{
    return served(Q, T, G, k_max, n_thr) ? lds_bytes(Q, T, G, k_max) : 0;
}

extern "C" int zira_phrase_match_f32(const float *prob, const float *boxes, const float *sizes, const uint32_t *phrase_bits,
                                     const float *gt_boxes, const int32_t *gt_count, int B, int Q, int T, int P, int G, int k_max,
                                     const double *iou_thrs, int n_thr, int merged, int32_t *top_query, float *top_score,
                                     double *top_iou, int32_t *first_hit, unsigned char *valid, void *stream)
{
    if (B < 1 || B > ZIRA_PHRASE_MAX_B || P < 1 || P > ZIRA_PHRASE_MAX_P || !served(Q, T, G, k_max, n_thr)) return ZIRA_MSDA_EINVAL;
    if (!prob || !boxes || !sizes || !phrase_bits || !gt_boxes || !gt_count || !iou_thrs || !top_query || !top_score || !top_iou ||
        !first_hit || !valid)
        return ZIRA_MSDA_EINVAL;
    PhraseArgs a = {};
    a.prob = prob, a.boxes = boxes, a.sizes = sizes, a.bits = phrase_bits, a.gt = gt_boxes, a.gt_count = gt_count;
    a.top_query = top_query, a.top_score = top_score, a.top_iou = top_iou, a.first_hit = first_hit, a.valid = valid;
    for (int t = 0; t < n_thr; ++t) a.thr[t] = iou_thrs[t];
    a.Q = Q, a.T = T, a.P = P, a.G = G, a.k_max = k_max, a.n_thr = n_thr, a.merged = merged != 0;
    a.net = network_size(Q);
    a.R = pow2_at_least(k_max < Q ? k_max : Q);
    a.vec = (T % 4 == 0) && (reinterpret_cast<uintptr_t>(prob) % 16 == 0);
    const int threads = a.net < 64 ? 64 : a.net;   // every entry of the network has its thread; k_max and the mask words fit in 64
    hipLaunchKernelGGL(phrase_match_kernel, dim3((unsigned)B * (unsigned)P), dim3((unsigned)threads), lds_bytes(Q, T, G, k_max),
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
