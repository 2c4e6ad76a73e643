// topk_select.h -- what topk.hip and vocab.hip share: the selection of the first k entries of the stable descending sort of a
// row (keys in LDS or re-read, radix select, compaction, bitonic sort of the survivors) and the evaluation tail that follows
// it (box to pixels of the output size, clip, drop empty, compact, zero behind the count).  One definition of each, so the
// merged tail of a chunked vocabulary (vocab.hip) is the detections tail (topk.hip) bit for bit.  Internal linkage.
#ifndef ZIRA_TOPK_SELECT_H_
#define ZIRA_TOPK_SELECT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stable_desc.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;
constexpr int kCopies = 8;               // histogram copies: 64 lanes on one digit (rows of one fill value, the exponent
                                         // digit of any row) are an 8-way LDS conflict instead of a 64-way one

// (key_of, the entry format and the sorting network: stable_desc.h)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t load_key(const uint32_t *keys, const float *__restrict__ x, int i)
{
    return IN_LDS ? keys[i] : key_of(x[i]);
}

__device__ __forceinline__ uint64_t lanes_below()
{
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

struct Shared {
    unsigned long long cand[kMaxK];   // the candidates, then the exchange buffer of the sort
    uint32_t hist[256 * kCopies];   // [digit][copy]
    uint32_t above[kWaves], equal[kWaves];
    uint32_t digit, skipped;
};

// -> this thread's entry of the sorted list (thread t holds rank t; 0 for t >= k): key << 32 | (0xFFFFFFFF - index)
template <bool IN_LDS>
__device__ __forceinline__ unsigned long long select_sorted(const float *__restrict__ x, int n, int k, int P, Shared &s,
                                                            uint32_t *keys)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (IN_LDS) {
        for (int i = t; i < n; i += kThreads) keys[i] = key_of(x[i]);
    }
    // ---- radix select: after the passes `prefix` is the k-th largest key and `need` of its copies belong to the answer
    uint32_t prefix = 0, need = (uint32_t)k;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = t; i < 256 * kCopies; i += kThreads) s.hist[i] = 0;
        __syncthreads();   // (also: the keys are in LDS)
        for (int i = t; i < n; i += kThreads) {
            const uint32_t key = load_key<IN_LDS>(keys, x, i);
            if ((key & himask) == prefix) atomicAdd(&s.hist[((key >> shift) & 255u) * kCopies + (lane & (kCopies - 1))], 1u);
        }
        __syncthreads();
        if (wave == 0) {   // the digit D with  #(digit > D) < need <= #(digit >= D): lane l scans digits 255 - 4 l ... 252 - 4 l
            uint32_t h[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[j] = 0;
#pragma unroll
                for (int c = 0; c < kCopies; ++c) h[j] += s.hist[(255 - (4 * lane + j)) * kCopies + c];
                sum += h[j];
            }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            uint32_t run = incl - sum;
            if (run < need && incl >= need) {   // exactly one lane
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (run < need && run + h[j] >= need) {
                        s.digit = 255u - (uint32_t)(4 * lane + j);
                        s.skipped = run;
                    }
                    run += h[j];
                }
            }
        }
        __syncthreads();
        prefix |= s.digit << shift;
        need -= s.skipped;
    }
    const uint32_t n_above = (uint32_t)k - need;

    // ---- candidates: every key above the threshold, and the first `need` (by index) equal to it
    const int seg = ((n + kWaves - 1) / kWaves + 63) & ~63;
    const int lo = wave * seg, hi = min(n, lo + seg);
    uint32_t c_above = 0, c_equal = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const uint32_t key = i < hi ? load_key<IN_LDS>(keys, x, i) : 0u;
        c_above += (uint32_t)__popcll(__ballot(i < hi && key > prefix));
        c_equal += (uint32_t)__popcll(__ballot(i < hi && key == prefix));
    }
    if (lane == 0) {
        s.above[wave] = c_above;
        s.equal[wave] = c_equal;
    }
    if (t >= k && t < P) s.cand[t] = 0ull;   // padding of the network: below every entry (no key is 0)
    __syncthreads();
    uint32_t at_above = 0, at_equal = 0;
    for (int w = 0; w < wave; ++w) {
        at_above += s.above[w];
        at_equal += s.equal[w];
    }
    const uint64_t below = lanes_below();
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const uint32_t key = i < hi ? load_key<IN_LDS>(keys, x, i) : 0u;
        const bool is_above = i < hi && key > prefix, is_equal = i < hi && key == prefix;
        const uint64_t ma = __ballot(is_above), me = __ballot(is_equal);
        const unsigned long long entry = ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)i);
        if (is_above) s.cand[at_above + (uint32_t)__popcll(ma & below)] = entry;
        if (is_equal) {
            const uint32_t r = at_equal + (uint32_t)__popcll(me & below);
            if (r < need) s.cand[n_above + r] = entry;
        }
        at_above += (uint32_t)__popcll(ma);
        at_equal += (uint32_t)__popcll(me);
    }
    __syncthreads();

    // ---- bitonic network over P = 2^p >= k entries, descending; thread t owns entry t
    const unsigned long long v = bitonic_desc(t < P ? s.cand[t] : 0ull, P, s.cand);
    return t < k ? v : 0ull;
}

inline int network_size(int k)
{
    int P = 1;
    while (P < k) P <<= 1;
    return P;
}

// ---- the box arithmetic of the evaluation tail, for every source that puts a query's box into a frame (the tail below,
// phrasematch.hip): cxcywh in 0..1 -> corners in pixels of the output size, clipped to it.  The float chain is the op chain's,
// every multiply / add / subtract rounded on its own (sx, sy: fl(out_w / img_w), fl(out_h / img_h)):
//   xyxy = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h);  x *= img_w, y *= img_h;  x *= sx, y *= sy;
//   x = min(max(x, 0), out_w), y likewise  (fmaxf / fminf: a NaN coordinate clips to 0).
__device__ __forceinline__ float4 box_to_output(const float4 box, float img_h, float img_w, float sx, float sy, float out_h,
                                                float out_w)
{
#pragma clang fp contract(off)
    const float hw = __fmul_rn(0.5f, box.z), hh = __fmul_rn(0.5f, box.w);
    float x0 = __fmul_rn(__fmul_rn(__fsub_rn(box.x, hw), img_w), sx);
    float y0 = __fmul_rn(__fmul_rn(__fsub_rn(box.y, hh), img_h), sy);
    float x1 = __fmul_rn(__fmul_rn(__fadd_rn(box.x, hw), img_w), sx);
    float y1 = __fmul_rn(__fmul_rn(__fadd_rn(box.y, hh), img_h), sy);
    x0 = fminf(fmaxf(x0, 0.f), out_w);
    x1 = fminf(fmaxf(x1, 0.f), out_w);
    y0 = fminf(fmaxf(y0, 0.f), out_h);
    y1 = fminf(fmaxf(y1, 0.f), out_h);
    return make_float4(x0, y0, x1, y1);
}

// ---- the evaluation tail behind a selection (GroundingDINO.dt_inference + structures.detector_postprocess): thread t of
// image b holds entry t of the selection where `live` (score, label, the address of its cxcywh box); the box goes to pixels
// of the requested output size, is clipped, and the entries whose box is not empty are compacted into row b of the k-wide
// outputs, zero at and behind their count.  The float chain is the op chain's, every multiply / add / subtract rounded on
// its own:
//   xyxy = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h);  x *= img_w, y *= img_h;  x *= fl(out_w / img_w), y *= fl(out_h / img_h);
//   x = min(max(x, 0), out_w), y likewise;  kept when x1 - x0 > 0 and y1 - y0 > 0.
// Every thread of the block calls it, after the last exchange of the sort.
__device__ __forceinline__ void detections_tail(bool live, float score, int64_t label, const float *__restrict__ box_at, int b, int k,
                                                const float *__restrict__ sizes, Shared &s, float *__restrict__ scores,
                                                int64_t *__restrict__ labels, float *__restrict__ xyxy,
                                                int32_t *__restrict__ n_keep)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float img_h = sizes[b * 4 + 0], img_w = sizes[b * 4 + 1], out_h = sizes[b * 4 + 2], out_w = sizes[b * 4 + 3];
    // the op chain divides two Python numbers (double) and rounds the quotient to fp32 when it meets the tensor
    const float sx = (float)((double)out_w / (double)img_w), sy = (float)((double)out_h / (double)img_h);
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    bool keep = false;
    if (live) {
        // (a NaN coordinate ends as a box that is not kept, whatever min / max make of it)
        const float4 px = box_to_output(*reinterpret_cast<const float4 *>(box_at), img_h, img_w, sx, sy, out_h, out_w);
        x0 = px.x, y0 = px.y, x1 = px.z, y1 = px.w;
        keep = __fsub_rn(x1, x0) > 0.f && __fsub_rn(y1, y0) > 0.f;
    }
    const uint64_t m = __ballot(keep);
    __syncthreads();   // (the last exchange of the sort has been read)
    if (lane == 0) s.above[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t at = 0, total = 0;
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = s.above[w];
        at += w < wave ? c : 0u;
        total += c;
    }
    at += (uint32_t)__popcll(m & lanes_below());
    const size_t o = (size_t)b * k;
    if (keep) {
        scores[o + at] = score;
        labels[o + at] = label;
        *reinterpret_cast<float4 *>(xyxy + (o + at) * 4) = make_float4(x0, y0, x1, y1);
    }
    if (t >= (int)total && t < k) {   // the unused tail is defined too
        scores[o + t] = 0.f;
        labels[o + t] = 0;
        *reinterpret_cast<float4 *>(xyxy + (o + t) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (t == 0) n_keep[b] = (int32_t)total;
}

}  // namespace

#endif  // ZIRA_TOPK_SELECT_H_
