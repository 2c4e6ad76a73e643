// grounding.hip -- the free-text grounding tail as ONE launch for a batch (C ABI: zira_ground_f32): the reference's
// `predict` chain  max(dim) -> > box_threshold -> prob[mask], boxes[mask] -> > text_threshold  with fixed-size padded outputs
// and a count per image in place of boolean-mask indexing, bit-identical to the chain.
//
// One 1024-thread block per image (the model has 900 queries and a batch of one or two: this is a latency kernel).
//   1. every wave walks its own queries (q = wave, wave + 16, ...): the 64 lanes read the row of T <= 256 probabilities -- as
//      one float4 per lane where T is a multiple of 4, as up to four coalesced scalars per lane otherwise -- and reduce
//      (value, index) to the row's maximum and its FIRST index; a NaN anywhere makes the score NaN (torch.max's rule).  The
//      lanes' `> text_threshold` compare bits become the row's W = ceil(T / 32) mask words.  Score, index and words stay in LDS;
//   2. thread q decides `score > box_threshold` (false for NaN) and the kept queries get their output position: by ballots
//      and a 16-entry scan in ascending q (order 0), or by the stable descending sort of stable_desc.h (order 1);
//   3. position p of every output is written from LDS through the position -> query table, zero at and behind n_keep.
// No global atomics, no workspace traffic, no host synchronisation, nothing that a replayed capture could find stale.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "stable_desc.h"
#include "zira_msda.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxB = 65535;
constexpr int kMaxQ = 1024;
constexpr int kMaxT = 256;
constexpr int kMaxW = kMaxT / 32;
constexpr size_t kWorkspace = 256;       // reserved: the kernel keeps its state on chip (0 must mean "not served")

struct Shared {
    unsigned long long exch[kMaxQ];      // the exchange buffer of the sort
    uint32_t words[kMaxQ * kMaxW];       // [q][W]
    float score[kMaxQ];
    int32_t arg[kMaxQ];
    int32_t src[kMaxQ];                  // output position -> query
    uint32_t count[kWaves];
};

// the larger value, equal values (-0.0 == +0.0) by the smaller index: torch.max(dim)'s choice among the numbers of a row
__device__ __forceinline__ void take_better(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// -> the row's (maximum, first index of it, holds-a-NaN) in every lane; lane w < W returns word w of the mask in `word`
template <bool VEC4>
__device__ __forceinline__ void scan_row(const float *__restrict__ row, int T, int W, float text_thr, float &best, int &besti,
                                         bool &nan, uint32_t &word)
{
    const int lane = threadIdx.x & 63;
    best = -INFINITY;
    besti = 0x7FFFFFFF;                  // (behind every token: a row of -inf still ends at index 0)
    bool has_nan = false;
    word = 0u;
    if (VEC4) {
        uint32_t nib = 0u;
        if (4 * lane < T) {              // T is a multiple of 4: all four or none
            const float4 x = *reinterpret_cast<const float4 *>(row + 4 * lane);
            const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                has_nan |= e[j] != e[j];
                take_better(best, besti, e[j], 4 * lane + j);
                nib |= (e[j] > text_thr ? 1u : 0u) << j;
            }
        }
        uint32_t part = nib << (4 * (lane & 7));      // the eight lanes 8 w ... 8 w + 7 hold word w
        part |= __shfl_xor(part, 1);
        part |= __shfl_xor(part, 2);
        part |= __shfl_xor(part, 4);
        word = __shfl(part, (lane & 7) * 8);          // lane w reads lane 8 w
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (64 * j < T) {            // (uniform)
                const int t = 64 * j + lane;
                const bool in = t < T;
                const float x = in ? row[t] : 0.f;
                if (in) {
                    has_nan |= x != x;
                    take_better(best, besti, x, t);
                }
                const uint64_t bal = __ballot(in && x > text_thr);      // tokens 64 j ... 64 j + 63: words 2 j and 2 j + 1
                if ((lane >> 1) == j) word = (uint32_t)(bal >> (32 * (lane & 1)));
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        take_better(best, besti, ov, oi);
    }
    nan = __ballot(has_nan) != 0ull;
    if (lane >= W) word = 0u;
}

template <bool VEC4>
__global__ __launch_bounds__(kThreads) void ground_kernel(const float *__restrict__ prob, const uint4 *__restrict__ boxes, int Q,
                                                          int T, int W, int P, float box_thr, float text_thr, int order,
                                                          int32_t *__restrict__ out_query, float *__restrict__ out_score,
                                                          uint4 *__restrict__ out_box, int32_t *__restrict__ out_arg,
                                                          uint32_t *__restrict__ out_bits, int32_t *__restrict__ n_keep)
{
    __shared__ Shared s;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t o = (size_t)b * Q;

    // ---- 1. per query: score, first index of it, mask words
    for (int q = wave; q < Q; q += kWaves) {
        float best;
        int besti;
        bool nan;
        uint32_t word;
        scan_row<VEC4>(prob + (o + q) * T, T, W, text_thr, best, besti, nan, word);
        if (lane == 0) {
            s.score[q] = nan ? __uint_as_float(0x7FC00000u) : best;
            s.arg[q] = besti;
        }
        if (lane < W) s.words[q * W + lane] = word;
    }
    __syncthreads();

    // ---- 2. the kept queries and their output positions
    const float sc = t < Q ? s.score[t] : 0.f;
    const bool keep = t < Q && sc > box_thr;         // strict; false for a NaN score
    const uint64_t m = __ballot(keep);
    if (lane == 0) s.count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t at = 0, total = 0;
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = s.count[w];
        at += w < wave ? c : 0u;
        total += c;
    }
    if (order == 0) {
        at += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (keep) s.src[at] = t;
    } else {
        // a kept score is a number, so its key is not 0: the queries that are not kept sink behind every kept one
        const unsigned long long v = bitonic_desc(keep ? entry_of(key_of(sc), (uint32_t)t) : 0ull, P, s.exch);
        if (t < (int)total) s.src[t] = (int32_t)index_of(v);
    }
    __syncthreads();

    // ---- 3. the outputs, position by position; zero at and behind `total`
    if (t < Q) {
        const bool live = t < (int)total;
        const int q = live ? s.src[t] : 0;
        out_query[o + t] = live ? q : 0;
        out_score[o + t] = live ? s.score[q] : 0.f;
        out_arg[o + t] = live ? s.arg[q] : 0;
        out_box[o + t] = live ? boxes[o + q] : make_uint4(0u, 0u, 0u, 0u);
    }
    for (int i = t; i < Q * W; i += kThreads) {
        const int p = i / W, w = i - p * W;
        out_bits[o * W + i] = p < (int)total ? s.words[s.src[p] * W + w] : 0u;
    }
    if (t == 0) n_keep[b] = (int32_t)total;
}

inline bool served(long long B, long long Q, long long T)
{
    return B >= 1 && B <= kMaxB && Q >= 1 && Q <= kMaxQ && T >= 1 && T <= kMaxT;
}

}  // namespace

extern "C" size_t zira_ground_workspace_bytes(int B, int Q, int T)
{
    return served(B, Q, T) ? kWorkspace : 0;
}

extern "C" int zira_ground_f32(const float *prob, const float *boxes, int B, int Q, int T, float box_threshold,
                               float text_threshold, int order, int32_t *query, float *score, float *box, int32_t *argmax_token,
                               uint32_t *token_bits, int32_t *n_keep, void *ws, size_t ws_bytes, void *stream)
{
    if (!prob || !boxes || !query || !score || !box || !argmax_token || !token_bits || !n_keep) return ZIRA_MSDA_EINVAL;
    if (!served(B, Q, T) || (order != 0 && order != 1) || !ws || ws_bytes < kWorkspace) return ZIRA_MSDA_EINVAL;
    if (((uintptr_t)boxes | (uintptr_t)box) & 15) return ZIRA_MSDA_EINVAL;   // rows of four floats move as one
    if (((uintptr_t)prob | (uintptr_t)score | (uintptr_t)query | (uintptr_t)argmax_token | (uintptr_t)token_bits |
         (uintptr_t)n_keep) & 3)
        return ZIRA_MSDA_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int W = (T + 31) / 32;
    int P = 1;
    while (P < Q) P <<= 1;
    const uint4 *boxes4 = reinterpret_cast<const uint4 *>(boxes);
    uint4 *box4 = reinterpret_cast<uint4 *>(box);
    if (T % 4 == 0 && ((uintptr_t)prob & 15) == 0)
        hipLaunchKernelGGL(ground_kernel<true>, dim3(B), dim3(kThreads), 0, st, prob, boxes4, Q, T, W, P, box_threshold,
                           text_threshold, order, query, score, box4, argmax_token, token_bits, n_keep);
    else
        hipLaunchKernelGGL(ground_kernel<false>, dim3(B), dim3(kThreads), 0, st, prob, boxes4, Q, T, W, P, box_threshold,
                           text_threshold, order, query, score, box4, argmax_token, token_bits, n_keep);
    return (int)hipGetLastError();
}
