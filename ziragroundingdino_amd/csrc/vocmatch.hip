// vocmatch.hip -- Pascal VOC box AP matching for a whole batch as ONE launch (C ABI: zira_voc_match): the detection walk of
// the reference's voc_eval for every image, label and IoU threshold, where the detections already are.  The rules (the text
// round trip's quantisation, the inclusive-pixel overlap, first-best GT, strict threshold, difficult GTs, duplicates) are
// stated at the declaration in include/zira_msda.h.
//
// voc_eval walks a label's detections in score order and keeps a `det` flag per GT, which looks sequential.  It is not: the GT
// a detection is compared with (jmax, the first GT of best overlap) does not depend on what was taken before, so
//     GT jmax is taken at threshold t when detection d arrives
//         <=>  an EARLIER detection d' of the image has jmax(d') == jmax(d) and ovmax(d') > thr_t.
// One block per image, thread k owns detection k (K <= 1024 = the block):
//   0. the block stages the image's GTs (corners, label, difficult) in LDS;
//   1. thread k quantises its detection, scans the GTs of its label (every lane reads the same GT: LDS broadcasts) for
//      ovmax / jmax, forms hit = the bits t with ovmax > thr_t, and leaves (order key, jmax, hit) in LDS;
//   2. thread k ORs the hits of the detections in front of it on the same GT (in front: larger order key, equal key smaller
//      row -- the ranking of stable_desc.h, on the fp64 qs), which gives TP = hit & ~seen, FP = the rest; a difficult jmax
//      gives neither.  Every output element is written once, with ordinary vector stores.
// No global atomics, no workspace, no allocation, no host synchronisation: the result depends on the inputs alone.
// Contraction is off for the whole file (and on the compile line): the union stays two products, an add and a subtract, and
// `x0 + 1.0f` stays an fp32 add on its own.
//
// Bound: launch latency plus one pass over the inputs and outputs -- per image K (4 + 8 + 16) + G (32 + 8 + 1) bytes read,
// K (8 + 4 + 4 + 4 T) written.  Beyond that a thread does one correctly rounded fp64 divide per GT of its label and K LDS reads
// of 16 bytes for the walk; with 20 labels at K = 300, G = 20 that is about one divide and 300 reads.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"
#include "zira_msda.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxB = 65535, kMaxK = 1024, kMaxG = 1024;

struct VocArgs {
    const float *scores;
    const int64_t *labels;
    const float *xyxy;
    const int32_t *n_keep;
    const double *gt_xyxy;
    const int64_t *gt_label;
    const unsigned char *gt_difficult;
    const int32_t *n_gt;
    double *qscore;
    uint32_t *tp, *fp;
    int32_t *gt_of;
    double thr[ZIRA_VOC_MAX_THRS];
    int K, G, T, num_classes;
};

// dynamic LDS: double gbox[G][4] | int64 key[K] | int2 jh[K] (jmax, hit) | int32 glab[G] | uint8 gdiff[G]
__host__ __device__ inline size_t lds_bytes(int K, int G)
{
    return (size_t)G * 32 + (size_t)K * 16 + (size_t)G * 4 + (size_t)G;
}

// Signed order == the order of the doubles, -0.0 == +0.0, NaN below every number (all NaNs equal).
__device__ __forceinline__ long long order_key(double q)
{
    if (q != q) return (long long)0x8000000000000000ull;
    if (q == 0.0) return 0;
    const long long b = __double_as_longlong(q);
    return b >= 0 ? b : -(b & 0x7FFFFFFFFFFFFFFFll);
}

__global__ __launch_bounds__(1024) void voc_match_kernel(const VocArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int K = a.K, G = a.G, T = a.T;

    double *gbox = reinterpret_cast<double *>(smem);
    long long *key = reinterpret_cast<long long *>(gbox + (size_t)G * 4);
    int2 *jh = reinterpret_cast<int2 *>(key + K);
    int32_t *glab = reinterpret_cast<int32_t *>(jh + K);
    unsigned char *gdiff = reinterpret_cast<unsigned char *>(glab + G);

    const int nk = min(max(a.n_keep[b], 0), K);
    const int ng = G > 0 ? min(max(a.n_gt[b], 0), G) : 0;
    const long long row = (long long)b * K, grow = (long long)b * G;
    const uint32_t all = T >= 32 ? 0xFFFFFFFFu : ((1u << T) - 1u);

    // ---- 0. stage the image's ground truth
    for (int g = tid; g < ng; g += nthreads) {
        const double *p = a.gt_xyxy + (grow + g) * 4;
        gbox[4 * g + 0] = p[0], gbox[4 * g + 1] = p[1], gbox[4 * g + 2] = p[2], gbox[4 * g + 3] = p[3];
        const int64_t c = a.gt_label[grow + g];
        glab[g] = c >= 0 && c < (int64_t)a.num_classes ? (int32_t)c : -1;     // -1: no detection that counts has it
        gdiff[g] = a.gt_difficult[grow + g] != 0;
    }
    __syncthreads();

    // ---- 1. per detection: the quantised box, ovmax / jmax, the hit bits
    for (int k = tid; k < K; k += nthreads) {
        double qs = 0.0;
        if (k < nk) {
            const float *p = a.xyxy + (row + k) * 4;
            qs = rint((double)a.scores[row + k] * 1000.0) / 1000.0;
            const float fx0 = p[0] + 1.0f, fy0 = p[1] + 1.0f;
            const double x0 = rint((double)fx0 * 10.0) / 10.0, y0 = rint((double)fy0 * 10.0) / 10.0;
            const double x1 = rint((double)p[2] * 10.0) / 10.0, y1 = rint((double)p[3] * 10.0) / 10.0;
            const int64_t c64 = a.labels[row + k];
            int jmax = -1;
            uint32_t hit = 0;
            if (c64 >= 0 && c64 < (int64_t)a.num_classes) {
                const int32_t c = (int32_t)c64;
                const double da = (x1 - x0 + 1.0) * (y1 - y0 + 1.0);
                double ovmax = -HUGE_VAL;
                for (int g = 0; g < ng; ++g) {
                    if (glab[g] != c) continue;
                    const double gx0 = gbox[4 * g + 0], gy0 = gbox[4 * g + 1], gx1 = gbox[4 * g + 2], gy1 = gbox[4 * g + 3];
                    const double iw = fmax(fmin(gx1, x1) - fmax(gx0, x0) + 1.0, 0.0);
                    const double ih = fmax(fmin(gy1, y1) - fmax(gy0, y0) + 1.0, 0.0);
                    const double inter = iw * ih;
                    const double uni = da + (gx1 - gx0 + 1.0) * (gy1 - gy0 + 1.0) - inter;
                    const double ov = inter / uni;
                    if (ov > ovmax) ovmax = ov, jmax = g;      // strict: the first of the best stays
                }
                for (int t = 0; t < T; ++t) hit |= (uint32_t)(ovmax > a.thr[t]) << t;
                // a label in range counts even without a GT: hit = 0, every bit an FP.  jmax = -2 marks a label out of range.
            } else {
                jmax = -2;
            }
            key[k] = order_key(qs);
            jh[k] = make_int2(jmax, (int)hit);
        }
        a.qscore[row + k] = qs;
    }
    __syncthreads();

    // ---- 2. per detection: what the detections in front of it took, and every output element once
    for (int k = tid; k < K; k += nthreads) {
        uint32_t tp = 0, fp = 0;
        int jmax = -1;
        if (k < nk) {
            const int2 me = jh[k];
            jmax = me.x;
            const uint32_t hit = (uint32_t)me.y;
            if (jmax != -2) {
                if (hit == 0u || jmax < 0) {       // (hit != 0 implies a GT was found)
                    fp = all;
                } else if (!gdiff[jmax]) {
                    const long long mine = key[k];
                    uint32_t seen = 0;
                    for (int j = 0; j < nk; ++j) {          // one address for the whole wave: broadcast reads
                        const int2 o = jh[j];
                        const long long theirs = key[j];
                        const bool front = theirs > mine || (theirs == mine && j < k);
                        seen |= (o.x == jmax && front) ? (uint32_t)o.y : 0u;
                    }
                    tp = hit & ~seen;
                    fp = all & ~tp;
                } else {
                    fp = all & ~hit;
                }
            }
        }
        a.tp[row + k] = tp, a.fp[row + k] = fp;
        if (a.gt_of) {
            int32_t *o = a.gt_of + (row + k) * T;
            for (int t = 0; t < T; ++t) o[t] = ((tp >> t) & 1u) ? jmax : -1;
        }
    }
}

}  // namespace

extern "C" int zira_voc_match(const float *scores, const int64_t *labels, const float *xyxy, const int32_t *n_keep, int B, int K,
                              const double *gt_xyxy, const int64_t *gt_label, const unsigned char *gt_difficult, const int32_t *n_gt,
                              int G, const double *thrs, int T, int num_classes, double *qscore, uint32_t *tp, uint32_t *fp,
                              int32_t *gt_of, void *stream)
{
    if (B < 1 || B > kMaxB || K < 1 || K > kMaxK || G < 0 || G > kMaxG || T < 1 || T > ZIRA_VOC_MAX_THRS || num_classes < 1)
        return ZIRA_MSDA_EINVAL;
    if (!scores || !labels || !xyxy || !n_keep || !thrs || !qscore || !tp || !fp) return ZIRA_MSDA_EINVAL;
    if (G > 0 && (!gt_xyxy || !gt_label || !gt_difficult || !n_gt)) return ZIRA_MSDA_EINVAL;
    VocArgs a = {};
    a.scores = scores, a.labels = labels, a.xyxy = xyxy, a.n_keep = n_keep;
    a.gt_xyxy = gt_xyxy, a.gt_label = gt_label, a.gt_difficult = gt_difficult, a.n_gt = n_gt;
    a.qscore = qscore, a.tp = tp, a.fp = fp, a.gt_of = gt_of;
    for (int t = 0; t < T; ++t) a.thr[t] = thrs[t];
    a.K = K, a.G = G, a.T = T, a.num_classes = num_classes;
    const int threads = ((K + 63) / 64) * 64;        // one thread per detection, whole waves
    const size_t lds = lds_bytes(K, G);              // at most 53 KB of a CU's 160 KB
    const hipError_t e = zira::lds_opt_in(voc_match_kernel, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)B), dim3((unsigned)threads), lds, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
