// lvismatch.hip -- LVIS box AP matching for a whole batch as ONE launch (C ABI: zira_lvis_match): lvis-api's per-image cut
// (LVISResults), its category filter (LVISEval._prepare) and LVISEval.evaluate_img for iou_type "bbox", where the detections
// already are.  The rules are stated in include/zira_lvis.h; the outputs are laid out as zira_ap_match's, so apaccum.hip serves
// them as it is.
//
// The launch is apmatch.hip's shape -- one block per image, one wave per (area range a, IoU threshold t) problem, up to 16
// waves, a block with more problems deals them round-robin -- with the federated rules in the staging step:
//   0. the block clears the image's positive-set words in LDS, stages the GTs (corners, box area, label, ignore bits per range)
//      and sets the bit of every GT label (an LDS `or`: the words do not depend on the order), then stages the first
//      min(n_keep, max_det) rows: a row whose label is outside 0..C-1 or in neither the positive set nor the image's neg_set
//      word keeps the label -1 and takes part in nothing; the others remember whether their label is in the nel_set word, and
//      count their rank among the earlier participating rows of their label;
//   1. per problem and detection: lanes are strided over the GTs (GT g belongs to lane g % 64; its matched bit is bit g / 64 of
//      a register), each lane tests label and availability, forms the IoU in fp64 and keeps its best candidate as an integer
//      key -- bit 63 = "not ignored", below it the IoU's bit pattern -- so that "the best not-ignored GT, else the best ignored
//      one" is one wave maximum; the largest original index among the lanes that hold the maximum wins the tie.  The flags of
//      32 detections collect in a register and go to LDS as one word per problem;
//   2. the block transposes the per-problem bit rows into one u64 per detection and writes every output element once, with
//      ordinary vector stores.
// No global atomics, no workspace, no allocation, no host synchronisation: the result depends on the inputs alone.
// Contraction is off for the whole file (and on the compile line): `da + ga - w * h` stays an add, a multiply and a subtract.
//
// Bound: launch latency plus one pass over the inputs and outputs (a few hundred KB for a batch); the serial chain of a wave
// (min(K, max_det) detections x ceil(A T / 16) problems, an LDS read, a divide and two wave reductions each) is what the launch
// costs beyond its latency.  A first version: nothing is tuned beyond "one launch, no sync".
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"
#include "zira_lvis.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxWaves = 16;
constexpr int kMaxBits = 64;

struct LvisArgs {
    const int64_t *labels;
    const float *xyxy;
    const int32_t *n_keep;
    const double *gt_xywh, *gt_area;
    const int64_t *gt_label;
    const unsigned char *gt_ignore;
    const int32_t *n_gt;
    const uint32_t *neg_set, *nel_set;
    int32_t *rank;
    unsigned long long *matched, *ignored;
    unsigned char *gt_ignored;
    int32_t *gt_of;
    double thr[ZIRA_AP_MAX_THRS];
    double lo[ZIRA_AP_MAX_AREAS], hi[ZIRA_AP_MAX_AREAS];
    int K, G, T, A, C, max_det;
};

// dynamic LDS: float4 dbox[K] | double gx0, gy0, gx1, gy1, garea [G] each | int32 glab[G] | int32 dlab[K] | int32 rank[K] |
// uint32 bits[A T][2][ceil(K / 32)] | uint32 pos[ceil(C / 32)] | uint8 gflag[G] | uint8 dnel[K]
inline size_t lds_bytes(int K, int G, int AT, int C)
{
    return (size_t)K * 16 + (size_t)G * 40 + (size_t)G * 4 + (size_t)K * 8 + (size_t)AT * 2 * ((K + 31) / 32) * 4 +
           (size_t)((C + 31) / 32) * 4 + (size_t)G + (size_t)K;
}

inline bool served(int K, int G, int T, int A, int C)
{
    return K >= 1 && K <= ZIRA_LVIS_MAX_K && G >= 0 && G <= ZIRA_LVIS_MAX_G && C >= 1 && C <= ZIRA_LVIS_MAX_CLASSES && T >= 1 &&
           T <= ZIRA_AP_MAX_THRS && A >= 1 && A <= ZIRA_AP_MAX_AREAS && A * T <= kMaxBits;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long y = __shfl_xor(v, o);
        v = y > v ? y : v;
    }
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kMaxWaves * 64) void lvis_match_kernel(const LvisArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = blockDim.x, nwaves = nthreads >> 6;
    const int K = a.K, G = a.G, T = a.T, AT = a.A * a.T, C = a.C, Kw = (K + 31) >> 5, W = (C + 31) >> 5;

    float4 *dbox = reinterpret_cast<float4 *>(smem);
    double *gx0 = reinterpret_cast<double *>(dbox + K), *gy0 = gx0 + G, *gx1 = gy0 + G, *gy1 = gx1 + G, *garea = gy1 + G;
    int32_t *glab = reinterpret_cast<int32_t *>(garea + G), *dlab = glab + G, *rank = dlab + K;
    uint32_t *bits = reinterpret_cast<uint32_t *>(rank + K), *pos = bits + (size_t)AT * 2 * Kw;
    unsigned char *gflag = reinterpret_cast<unsigned char *>(pos + W), *dnel = gflag + G;

    const int nk = min(min(max(a.n_keep[b], 0), K), a.max_det);      // the image cut: the first max_det rows of the image
    const int ng = G > 0 ? min(max(a.n_gt[b], 0), G) : 0;
    const long long row = (long long)b * K, grow = (long long)b * G, srow = (long long)b * W;

    // ---- 0. stage the image
    for (int w = tid; w < W; w += nthreads) pos[w] = 0u;
    __syncthreads();
    for (int g = tid; g < ng; g += nthreads) {
        const double *p = a.gt_xywh + (grow + g) * 4;
        const double x = p[0], y = p[1], w = p[2], h = p[3], area = a.gt_area[grow + g];
        gx0[g] = x, gy0[g] = y, gx1[g] = x + w, gy1[g] = y + h, garea[g] = w * h;
        const int64_t c = a.gt_label[grow + g];
        const bool in_c = c >= 0 && c < (int64_t)C;
        glab[g] = in_c ? (int32_t)c : -2;                             // -2: the label of no detection
        if (in_c) atomicOr(&pos[(int)c >> 5], 1u << ((int)c & 31));   // LDS: the positive set, ignored GTs included
        const bool ign = a.gt_ignore[grow + g] != 0;
        unsigned f = 0u;
        for (int ai = 0; ai < a.A; ++ai) f |= (unsigned)(ign || area < a.lo[ai] || area > a.hi[ai]) << ai;
        gflag[g] = (unsigned char)f;
    }
    __syncthreads();
    for (int k = tid; k < nk; k += nthreads) {
        const float *p = a.xyxy + (row + k) * 4;
        dbox[k] = make_float4(p[0], p[1], p[2], p[3]);
        const int64_t c = a.labels[row + k];
        int32_t keep = -1;
        unsigned char nel = 0;
        if (c >= 0 && c < (int64_t)C) {
            const int w = (int)c >> 5, s = (int)c & 31;
            if (((pos[w] | a.neg_set[srow + w]) >> s) & 1u) keep = (int32_t)c;
            nel = (unsigned char)((a.nel_set[srow + w] >> s) & 1u);
        }
        dlab[k] = keep, dnel[k] = nel;
    }
    __syncthreads();
    for (int k = tid; k < nk; k += nthreads) {   // dlab[j] is one address for the whole wave: a broadcast read
        const int32_t c = dlab[k];
        int cnt = 0;
        for (int j = 0; j < k; ++j) cnt += dlab[j] == c;
        rank[k] = c >= 0 ? cnt : -1;
    }
    __syncthreads();

    // ---- 1. the problems, one wave each
    for (int p = wave; p < AT; p += nwaves) {
        const int ai = p / T, ti = p - ai * T;
        const double thr = fmin(a.thr[ti], 1.0 - 1e-10), lo = a.lo[ai], hi = a.hi[ai];
        uint32_t *pm = bits + (size_t)p * 2 * Kw, *pi = pm + Kw;
        uint32_t taken = 0;                 // bit j: GT lane + 64 j is matched
        uint32_t mw = 0, iw = 0;            // the flags of detections k & ~31 ... k
        for (int k = 0; k < nk; ++k) {
            int m = -1;
            const int32_t c = dlab[k];
            if (c >= 0) {
                const float4 box = dbox[k];
                const double dx = box.x, dy = box.y, dw = (double)(box.z - box.x), dh = (double)(box.w - box.y);
                const double da = dw * dh, dx1 = dx + dw, dy1 = dy + dh;
                unsigned long long key = 0;   // 0: no candidate; else ((not ignored) << 63 | bits of the IoU) + 1
                int best_g = -1;
                for (int j = 0, g = lane; g < ng; ++j, g += 64) {
                    if (glab[g] != c || ((taken >> j) & 1u)) continue;
                    double iou = 0.0;
                    const double w = fmin(dx1, gx1[g]) - fmax(dx, gx0[g]);
                    if (w > 0.0) {
                        const double h = fmin(dy1, gy1[g]) - fmax(dy, gy0[g]);
                        if (h > 0.0) {
                            const double i = w * h;
                            const double u = da + garea[g] - i;
                            iou = i / u;
                        }
                    }
                    if (iou < thr) continue;
                    const unsigned long long cand =
                        (((unsigned long long)__double_as_longlong(iou) & 0x7FFFFFFFFFFFFFFFull) |
                         (((gflag[g] >> ai) & 1u) ? 0ull : 0x8000000000000000ull)) + 1ull;
                    if (cand >= key) key = cand, best_g = g;   // equal IoU: the later GT
                }
                const unsigned long long top = wave_max(key);
                bool ign;
                if (top != 0ull) {
                    m = wave_max(key == top ? best_g : -1);
                    ign = ((top - 1ull) >> 63) == 0ull;
                    if ((m & 63) == lane) taken |= 1u << (m >> 6);
                } else {
                    ign = da < lo || da > hi || dnel[k] != 0;    // the last: LVIS's not-exhaustive rule
                }
                mw |= (uint32_t)(m >= 0) << (k & 31);
                iw |= (uint32_t)ign << (k & 31);
            }
            if (a.gt_of && lane == 0) a.gt_of[(row + k) * AT + p] = m;
            if ((k & 31) == 31 || k == nk - 1) {
                if (lane == 0) pm[k >> 5] = mw, pi[k >> 5] = iw;
                mw = iw = 0;
            }
        }
    }
    __syncthreads();

    // ---- 2. every output element once
    for (int k = tid; k < K; k += nthreads) {
        int r = -1;
        unsigned long long M = 0, I = 0;
        if (k < nk) {
            r = rank[k];
            const uint32_t *w = bits + (k >> 5);
            for (int p = 0; p < AT; ++p) {
                M |= (unsigned long long)((w[(size_t)p * 2 * Kw] >> (k & 31)) & 1u) << p;
                I |= (unsigned long long)((w[(size_t)p * 2 * Kw + Kw] >> (k & 31)) & 1u) << p;
            }
        }
        a.rank[row + k] = r, a.matched[row + k] = M, a.ignored[row + k] = I;
    }
    for (int g = tid; g < G; g += nthreads) a.gt_ignored[grow + g] = g < ng ? gflag[g] : (unsigned char)0;
    if (a.gt_of) {
        int32_t *tail = a.gt_of + (row + nk) * AT;
        const long long n = (long long)(K - nk) * AT;
        for (long long i = tid; i < n; i += nthreads) tail[i] = -1;
    }
}

}  // namespace

extern "C" size_t zira_lvis_match_lds_bytes(int K, int G, int T, int A, int C)
{
    return served(K, G, T, A, C) ? lds_bytes(K, G, A * T, C) : 0;
}

extern "C" int zira_lvis_match(const float *scores, const int64_t *labels, const float *xyxy, const int32_t *n_keep, int B, int K,
                               const double *gt_xywh, const double *gt_area, const int64_t *gt_label,
                               const unsigned char *gt_ignore, const int32_t *n_gt, int G, const uint32_t *neg_set,
                               const uint32_t *nel_set, int C, const double *iou_thrs, int T, const double *area_rng, int A,
                               int max_det, int32_t *rank, uint64_t *matched, uint64_t *ignored, unsigned char *gt_ignored,
                               int32_t *gt_of, void *stream)
{
    if (B < 1 || B > ZIRA_LVIS_MAX_B || !served(K, G, T, A, C) || max_det < 1 || max_det > K) return ZIRA_MSDA_EINVAL;
    if (!scores || !labels || !xyxy || !n_keep || !neg_set || !nel_set || !iou_thrs || !area_rng || !rank || !matched || !ignored)
        return ZIRA_MSDA_EINVAL;
    if (G > 0 && (!gt_xywh || !gt_area || !gt_label || !gt_ignore || !n_gt || !gt_ignored)) return ZIRA_MSDA_EINVAL;
    LvisArgs a = {};
    a.labels = labels, a.xyxy = xyxy, a.n_keep = n_keep;
    a.gt_xywh = gt_xywh, a.gt_area = gt_area, a.gt_label = gt_label, a.gt_ignore = gt_ignore, a.n_gt = n_gt;
    a.neg_set = neg_set, a.nel_set = nel_set;
    a.rank = rank, a.matched = reinterpret_cast<unsigned long long *>(matched);
    a.ignored = reinterpret_cast<unsigned long long *>(ignored), a.gt_ignored = gt_ignored, a.gt_of = gt_of;
    for (int t = 0; t < T; ++t) a.thr[t] = iou_thrs[t];
    for (int i = 0; i < A; ++i) a.lo[i] = area_rng[2 * i], a.hi[i] = area_rng[2 * i + 1];
    a.K = K, a.G = G, a.T = T, a.A = A, a.C = C, a.max_det = max_det;
    const int AT = A * T, waves = AT < kMaxWaves ? AT : kMaxWaves;
    const size_t lds = lds_bytes(K, G, AT, C);    // at most 88 KB of a CU's 160 KB
    const hipError_t e = zira::lds_opt_in(lvis_match_kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lvis_match_kernel, dim3((unsigned)B), dim3((unsigned)(waves * 64)), lds, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
