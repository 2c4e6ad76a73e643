/*
 * zira_lvis.h -- C ABI of the LVIS box AP matching for federated category lists (csrc/lvismatch.hip), a public header of
 * libzira_msda.so beside zira_msda.h.  Semantics: lvis-api's LVISResults (the per-image cut) and LVISEval._prepare /
 * evaluate_img for iou_type "bbox" over a whole batch -- what the reference's LVISEvaluator gets from the `lvis` package and this
 * stack does not have.  The output is laid out as zira_ap_match lays its own out, so zira_ap_accumulate serves it unchanged
 * with max_dets = (max_det).
 *
 * Inputs.  Detections as zira_detections_f32 / zira_det_merge_f32 write them: scores [B, K] fp32 (not read: the rows ARE in
 * non-increasing score order, the caller's precondition), labels [B, K] i64, xyxy [B, K, 4] fp32, n_keep [B] i32 (values outside
 * 0..K are clamped).  Ground truth padded to G per image: gt_xywh [B, G, 4] fp64 (x, y, w, h), gt_area [B, G] fp64, gt_label
 * [B, G] i64, gt_ignore [B, G] u8 (the annotation's own `ignore` flag; LVIS has no crowd), n_gt [B] i32 (clamped to 0..G); with
 * G == 0 the five (and gt_ignored) may be null.  Two category bitsets per image, neg_set and nel_set [B, W] u32, W =
 * ceil(C / 32), category c at bit c % 32 of word c / 32: the image's neg_category_ids and not_exhaustive_category_ids; bits at
 * and above C are never looked at.  The image's positive set is formed inside the launch from the labels of its first n_gt[b]
 * GTs, ignored ones included (a GT label outside 0..C-1 is in no set).  iou_thrs: T (1..ZIRA_AP_MAX_THRS) doubles, area_rng: A
 * (1..ZIRA_AP_MAX_AREAS) pairs (lo, hi) of doubles, both in HOST memory, read during the call and handed to the kernel by value.
 *
 * Rules, per image b:
 *   - image cut: only the first min(n_keep[b], max_det) rows take part -- the stable top max_det by score over all categories
 *     (LVISResults cuts to 300 per image; COCOeval cuts per class);
 *   - category filter: a detection takes part only if its label is in 0..C-1 and in the image's positive or negative set (a
 *     category that was never checked on the image is not a false positive); every other row has rank = -1 and zero bits;
 *   - GT list of (b, label, area range a): a GT is ignored for a when its `ignore` flag is set or area < lo_a or area > hi_a; the
 *     list is the not-ignored GTs in original order, then the ignored ones in original order (a stable sort);
 *   - IoU in fp64, every operation rounded on its own (no contraction), as at zira_ap_match with crowd = 0 everywhere:
 *     dw = (double)fl32(x1 - x0), dh likewise, da = dw dh, ga = gw gh, w = fmin(dx + dw, gx + gw) - fmax(dx, gx), h likewise,
 *     iou = 0 where w <= 0 or h <= 0, else i = w h, iou = i / (da + ga - i);
 *   - greedy walk per threshold t, the detections in row order: best = fmin(thr_t, 1 - 1e-10); scan the list, skipping a GT
 *     that is already matched, stopping at the first ignored GT once a not-ignored one is held, skipping iou < best, else
 *     best = iou and the GT is held (equal IoU: the LATER one wins).  A held GT sets the detection's matched bit, hands it its
 *     ignore flag and is matched from then on;
 *   - an unmatched detection is ignored when da < lo_a or da > hi_a or its label is in the image's nel_set (the LVIS rule: a
 *     category that was not exhaustively annotated on the image yields no false positives).
 *
 * Outputs, every element written exactly once: rank [B, K] i32 = the number of earlier PARTICIPATING detections of the image
 * with the same label, -1 for a row that does not take part;  matched / ignored [B, K] u64, bit a T + t, zero where rank is -1;
 * gt_ignored [B, G] u8, bit a, zero behind n_gt[b];  gt_of [B, K, A T] i32 (nullable) = the matched GT's original index or -1.
 *
 * General contract (as zira_msda.h): device pointers to contiguous arrays, aligned to their element type; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream); the entry only enqueues ONE launch, never synchronises, allocates
 * nothing, needs no workspace and is capturable into a hipGraph; no global atomics: the result depends on the inputs alone, two
 * calls give the same bits.  Served: 1 <= B <= ZIRA_LVIS_MAX_B, 1 <= K <= ZIRA_LVIS_MAX_K, 0 <= G <= ZIRA_LVIS_MAX_G,
 * 1 <= C <= ZIRA_LVIS_MAX_CLASSES, A T <= 64, 1 <= max_det <= K; anything else, or a null pointer other than gt_of (and the GT
 * arrays with G == 0), returns ZIRA_MSDA_EINVAL: host arithmetic, nothing is launched.  Return 0, ZIRA_MSDA_EINVAL or a
 * hipError_t cast to int.
 */
#ifndef ZIRA_LVIS_H_
#define ZIRA_LVIS_H_

#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h" /* ZIRA_MSDA_EINVAL, ZIRA_AP_MAX_THRS, ZIRA_AP_MAX_AREAS */

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_LVIS_MAX_B 65535
#define ZIRA_LVIS_MAX_K 1024
#define ZIRA_LVIS_MAX_G 1024
#define ZIRA_LVIS_MAX_CLASSES 65535

/* bytes of dynamic LDS the launch takes per block (host arithmetic; above 48 KB the entry opts in by itself); 0: a shape the
 * kernel declines */
size_t zira_lvis_match_lds_bytes(int K, int G, int T, int A, int C);

int zira_lvis_match(const float *scores, const int64_t *labels, const float *xyxy, const int32_t *n_keep, int B, int K,
                    const double *gt_xywh, const double *gt_area, const int64_t *gt_label, const unsigned char *gt_ignore,
                    const int32_t *n_gt, int G, const uint32_t *neg_set, const uint32_t *nel_set, int C, const double *iou_thrs,
                    int T, const double *area_rng, int A, int max_det, int32_t *rank, uint64_t *matched, uint64_t *ignored,
                    unsigned char *gt_ignored, int32_t *gt_of, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_LVIS_H_ */
