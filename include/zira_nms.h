/*
 * zira_nms.h -- C ABI of the batched box NMS behind the detection and grounding tails (csrc/nms.hip), a public header of
 * libzira_msda.so beside zira_msda.h.  Semantics: torchvision.ops.nms per image and, with labels, _batched_nms_vanilla --
 * what the reference's model files import from torchvision and this stack does not have.
 *
 * Per image b, over the first n[b] rows of its K:
 *   - the candidates are visited in the stable descending order of their scores (csrc/stable_desc.h: equal scores by ascending
 *     index, -0.0 == +0.0, NaN first);
 *   - candidate i is kept unless an earlier KEPT candidate j has iou(i, j) > iou_threshold (strict; a NaN IoU, 0 / 0 from two
 *     empty boxes, compares false) and, where `labels` is given, labels[j] == labels[i];
 *   - iou = inter / (area_i + area_j - inter), inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)),
 *     area = (x2 - x1) * (y2 - y1): fp32, every operation rounded on its own, the divide correctly rounded.
 *
 * General contract (as zira_msda.h):
 *   - device pointers to contiguous arrays: boxes [B, K, 4] fp32 xyxy (16-byte aligned), scores [B, K] fp32, labels [B, K]
 *     int64 (8-byte aligned) or NULL for class-agnostic suppression, n [B] int32 -- the counts zira_detections_f32 /
 *     zira_ground_f32 write; a count below 0 is read as 0, one above K as K.  Rows at and behind n[b] are never read;
 *   - keep [B, K] int32: the kept indices of image b in descending score order, -1 behind them; n_keep [B] int32: their count;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry only enqueues ONE launch, never
 *     synchronises, allocates nothing, needs no workspace and is capturable into a hipGraph;
 *   - no atomics of any kind: the result is a function of the input alone, two calls give the same bits;
 *   - return value: 0, ZIRA_MSDA_EINVAL (a null or misaligned pointer other than `labels`, B outside 1 .. ZIRA_NMS_MAX_B, K
 *     outside 1 .. ZIRA_NMS_MAX_K: host arithmetic, nothing is launched) or a hipError_t cast to int.
 */
#ifndef ZIRA_NMS_H_
#define ZIRA_NMS_H_

#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h" /* ZIRA_MSDA_EINVAL */

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_NMS_MAX_K 1024
#define ZIRA_NMS_MAX_B 65535

/* bytes of LDS the launch for K candidates takes per block (host arithmetic); 0: a K the kernel declines */
size_t zira_nms_lds_bytes(int K);

int zira_nms_f32(const float *boxes, const float *scores, const int64_t *labels, const int32_t *n, int B, int K,
                 float iou_threshold, int32_t *keep, int32_t *n_keep, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_NMS_H_ */
