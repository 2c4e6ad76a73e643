// apaccum.hip -- COCO box AP accumulation as ONE launch (C ABI: zira_ap_accumulate): the second half of pycocotools'
// COCOeval.accumulate over the state zira_ap_match left on the device.  The rules are stated at the declaration in
// include/zira_msda.h; the arithmetic is integer prefix counts, two fp64 divides and one fp64 add per kept detection and
// comparisons, so the tables are the host's (evaluation.accumulate) bit for bit.
//
// One block per cell (class c, area range a, max-det index mi), one wave per IoU threshold t.  The caller has put the
// detections in order (class after class, score order inside a class), so a wave walks its class's segment once, 64
// detections a step:
//   1. a lane tests its detection (rank under the cut, ignore bit clear -> kept; matched bit -> hit); two ballots and two
//      popcounts under the lane's mask give its inclusive counts, the carries of the earlier steps ride in registers;
//   2. a kept lane forms rc and pr, finds by bisection how many recall thresholds are <= rc (its bucket, 0..R) and raises the
//      bucket's maximum in LDS -- a precision is a non-negative double, so its bit pattern orders as an unsigned integer and
//      the maximum is one 64-bit LDS integer maximum.  Bucket 0 (rc under every threshold) feeds nothing and is not kept;
//   3. after the walk, precision at r is the maximum of the buckets above r: lanes take r = lane, lane + 64, ... and read up.
// "pr[j] for the first j with rc[j] >= thr, after the reverse running maximum" of the host is "the maximum of pr[j] over
// rc[j] >= thr" because rc never decreases -- no reverse pass, no stored curve.
// No global atomics, no workspace, no allocation, no host synchronisation; every output element is written once, with
// ordinary vector stores.  Contraction is off for the whole file (and on the compile line): tp + fp + eps stays an add.
//
// Bound: launch latency plus A M T passes over a class's 20 bytes per detection (L2 hits after the first) and one pass over
// the tables; the serial chain is a wave's ceil(n_c / 64) steps of the largest class.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h"

#pragma clang fp contract(off)

namespace {

struct AccArgs {
    const int32_t *rank;
    const unsigned long long *matched, *ignored;
    const int64_t *seg_off;
    const int32_t *npig;
    double *precision, *recall;
    long long n;
    int C, T, A, M, R;
    int32_t max_dets[ZIRA_AP_MAX_DETS];
    double rec_thrs[ZIRA_AP_MAX_RECS];
};

// LDS: double thr[R] | u64 best[T][R + 1]  (at most 2 KB + 16 * 257 * 8 = 34.9 KB: under the 48 KB that need no opt-in)
constexpr int kLdsWords = ZIRA_AP_MAX_RECS + ZIRA_AP_MAX_THRS * (ZIRA_AP_MAX_RECS + 1);

__global__ __launch_bounds__(ZIRA_AP_MAX_THRS * 64) void ap_accumulate_kernel(const AccArgs a)
{
    __shared__ unsigned long long smem[kLdsWords];
    const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6, nthreads = blockDim.x;   // blockDim.x == 64 T
    const int C = a.C, T = a.T, A = a.A, M = a.M, R = a.R;
    const int cell = blockIdx.x, mi = cell % M, ai = (cell / M) % A, c = cell / (M * A);

    double *thr = reinterpret_cast<double *>(smem);
    unsigned long long *best = smem + R + (size_t)t * (R + 1);      // this wave's row

    const long long rstride = (long long)C * A * M;                  // precision[t][r + 1] - precision[t][r]
    const long long at_c = ((long long)c * A + ai) * M + mi;
    double *const p_out = a.precision + (long long)t * R * rstride + at_c;
    double *const r_out = a.recall + (long long)t * rstride + at_c;

    const int npig = a.npig[c * A + ai];
    if (npig <= 0) {                                                 // the whole block leaves together
        for (int r = lane; r < R; r += 64) p_out[r * rstride] = -1.0;
        if (lane == 0) *r_out = -1.0;
        return;
    }

    for (int r = tid; r < R; r += nthreads) thr[r] = a.rec_thrs[r];
    for (int i = tid; i < T * (R + 1); i += nthreads) smem[R + i] = 0ull;
    __syncthreads();

    const long long n = a.n;
    long long lo = a.seg_off[c], hi = a.seg_off[c + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    const int max_det = a.max_dets[mi], bit = ai * T + t;
    const double gts = (double)npig;
    const unsigned long long upto = ~0ull >> (63 - lane);            // lanes 0 .. lane
    long long kept = 0, hits = 0;                                    // of the steps behind

    for (long long base = lo; base < hi; base += 64) {
        const long long i = base + lane;
        bool keep = false, hit = false;
        if (i < hi) {
            const int rk = a.rank[i];
            const unsigned long long ig = a.ignored[i], ma = a.matched[i];
            keep = rk >= 0 && rk < max_det && ((ig >> bit) & 1ull) == 0ull;
            hit = keep && ((ma >> bit) & 1ull) != 0ull;
        }
        const unsigned long long km = __ballot(keep), hm = __ballot(hit);
        if (keep) {
            const long long k_in = kept + __popcll(km & upto), h_in = hits + __popcll(hm & upto);
            const double tp = (double)h_in, fp = (double)(k_in - h_in);
            const double rc = tp / gts;
            const double pr = tp / (tp + fp + 0x1p-52);
            int b = 0, len = R;                                      // b = the number of thresholds <= rc
            while (len > 0) {
                const int half = len >> 1;
                if (thr[b + half] <= rc) b += half + 1, len -= half + 1;
                else len = half;
            }
            if (b > 0) atomicMax(best + b, (unsigned long long)__double_as_longlong(pr));
        }
        kept += __popcll(km), hits += __popcll(hm);
    }
    __syncthreads();

    if (lane == 0) *r_out = kept > 0 ? (double)hits / gts : 0.0;
    for (int r = lane; r < R; r += 64) {
        unsigned long long q = 0ull;
        for (int b = r + 1; b <= R; ++b) q = best[b] > q ? best[b] : q;
        p_out[r * rstride] = __longlong_as_double((long long)q);
    }
}

}  // namespace

extern "C" int zira_ap_accumulate(const int32_t *rank, const uint64_t *matched, const uint64_t *ignored, long long n,
                                  const int64_t *seg_off, const int32_t *npig, int C, int T, int A, const int32_t *max_dets, int M,
                                  const double *rec_thrs, int R, double *precision, double *recall, void *stream)
{
    if (C < 1 || C > ZIRA_AP_MAX_CLASSES || T < 1 || T > ZIRA_AP_MAX_THRS || A < 1 || A > ZIRA_AP_MAX_AREAS || A * T > 64)
        return ZIRA_MSDA_EINVAL;
    if (M < 1 || M > ZIRA_AP_MAX_DETS || R < 1 || R > ZIRA_AP_MAX_RECS || n < 0 || n > 0x7FFFFFFFll) return ZIRA_MSDA_EINVAL;
    if (!seg_off || !npig || !max_dets || !rec_thrs || !precision || !recall) return ZIRA_MSDA_EINVAL;
    if (n > 0 && (!rank || !matched || !ignored)) return ZIRA_MSDA_EINVAL;
    AccArgs a = {};
    for (int m = 0; m < M; ++m) {
        if (max_dets[m] < 1) return ZIRA_MSDA_EINVAL;
        a.max_dets[m] = max_dets[m];
    }
    for (int r = 0; r < R; ++r) {
        if (r > 0 && !(rec_thrs[r] >= rec_thrs[r - 1])) return ZIRA_MSDA_EINVAL;     // ascending (and no NaN)
        a.rec_thrs[r] = rec_thrs[r];
    }
    if (!(rec_thrs[0] == rec_thrs[0])) return ZIRA_MSDA_EINVAL;
    a.rank = rank, a.matched = reinterpret_cast<const unsigned long long *>(matched);
    a.ignored = reinterpret_cast<const unsigned long long *>(ignored);
    a.seg_off = seg_off, a.npig = npig, a.precision = precision, a.recall = recall;
    a.n = n, a.C = C, a.T = T, a.A = A, a.M = M, a.R = R;
    hipLaunchKernelGGL(ap_accumulate_kernel, dim3((unsigned)(C * A * M)), dim3((unsigned)(T * 64)), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
