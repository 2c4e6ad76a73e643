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
#include "stable_desc.h"
#include "zira_msda.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;
constexpr int kMaxN = 1 << 20;
constexpr int kMaxRows = 65535;
constexpr int kLdsMaxN = 32768;          // 128 KB of keys beside 17 KB of static LDS, of a CU's 160 KB
constexpr int kCopies = 8;               // histogram copies: 64 lanes on one digit (rows of one fill value, the exponent
                                         // digit of any row) are an 8-way LDS conflict instead of a 64-way one
constexpr size_t kWorkspace = 256;       // reserved: the kernels keep their state on chip (0 must mean "not served")

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
// empty ones dropped (GroundingDINO.dt_inference + structures.detector_postprocess).  The float chain is the op chain's,
// every multiply / add / subtract rounded on its own:
//   xyxy = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h);  x *= img_w, y *= img_h;  x *= fl(out_w / img_w), y *= fl(out_h / img_h);
//   x = min(max(x, 0), out_w), y likewise;  kept when x1 - x0 > 0 and y1 - y0 > 0.
template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void detections_kernel(const float *__restrict__ prob, const float *__restrict__ boxes,
                                                              int Q, int C, int k, int P, const float *__restrict__ sizes,
                                                              float *__restrict__ scores, int64_t *__restrict__ labels,
                                                              float *__restrict__ xyxy, int32_t *__restrict__ n_keep)
{
#pragma clang fp contract(off)
    extern __shared__ uint32_t keys[];
    __shared__ Shared s;
    const int b = blockIdx.x, n = Q * C;
    const float *row = prob + (size_t)b * n;
    const unsigned long long v = select_sorted<IN_LDS>(row, n, k, P, s, keys);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

    const float img_h = sizes[b * 4 + 0], img_w = sizes[b * 4 + 1], out_h = sizes[b * 4 + 2], out_w = sizes[b * 4 + 3];
    // the op chain divides two Python numbers (double) and rounds the quotient to fp32 when it meets the tensor
    const float sx = (float)((double)out_w / (double)img_w), sy = (float)((double)out_h / (double)img_h);
    float score = 0.f, x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    int64_t label = 0;
    bool keep = false;
    if (t < k) {
        const uint32_t idx = 0xFFFFFFFFu - (uint32_t)v;
        const uint32_t q = idx / (uint32_t)C;
        label = (int64_t)(idx - q * (uint32_t)C);
        score = row[idx];
        const float4 box = *reinterpret_cast<const float4 *>(boxes + ((size_t)b * Q + q) * 4);
        const float hw = __fmul_rn(0.5f, box.z), hh = __fmul_rn(0.5f, box.w);
        x0 = __fmul_rn(__fmul_rn(__fsub_rn(box.x, hw), img_w), sx);
        y0 = __fmul_rn(__fmul_rn(__fsub_rn(box.y, hh), img_h), sy);
        x1 = __fmul_rn(__fmul_rn(__fadd_rn(box.x, hw), img_w), sx);
        y1 = __fmul_rn(__fmul_rn(__fadd_rn(box.y, hh), img_h), sy);
        // (a NaN coordinate ends as a box that is not kept, whatever min / max make of it)
        x0 = fminf(fmaxf(x0, 0.f), out_w);
        x1 = fminf(fmaxf(x1, 0.f), out_w);
        y0 = fminf(fmaxf(y0, 0.f), out_h);
        y1 = fminf(fmaxf(y1, 0.f), out_h);
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

inline bool served(long long rows, long long n, long long k)
{
    return rows >= 1 && rows <= kMaxRows && k >= 1 && k <= kMaxK && n >= k && n <= kMaxN;
}

inline int network_size(int k)
{
    int P = 1;
    while (P < k) P <<= 1;
    return P;
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
