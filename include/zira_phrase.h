/*
 * zira_phrase.h -- C ABI of the phrase-grounding matching (csrc/phrasematch.hip), a public header of libzira_msda.so beside
 * zira_msda.h.  It scores what GroundingDINO.forward_grounding returns against annotated phrases: per (image, phrase) the best
 * k_max queries by the phrase's score, the best IoU of each with the phrase's ground-truth boxes, and per IoU threshold the rank
 * of the first hit -- what Flickr30k-Entities-style Recall@k and RefCOCO-style Precision@IoU are counted from.  The reference
 * has no evaluator of this kind; the definition is this header's (and phrase_evaluation.match_reference's, the same rules as
 * torch ops).
 *
 * Inputs.  prob [B, Q, T] fp32 (token probabilities) and boxes [B, Q, 4] fp32 (cx, cy, w, h in 0..1), as forward_grounding gives
 * them; sizes [B, 2] fp32 = (h, w), the frame the ground-truth boxes live in; phrase_bits [B, P, W] u32, W = ceil(T / 32), token
 * t at bit t % 32 of word t / 32 (the layout of zira_ground_f32's token_bits; bits at and above T are never looked at);
 * gt_boxes [B, P, G, 4] fp32, absolute (x0, y0, x1, y1); gt_count [B, P] i32 (clamped to 0..G): the first gt_count boxes of a
 * phrase are real.  iou_thrs: n_thr (1..ZIRA_PHRASE_MAX_THRS) doubles in HOST memory, read during the call and handed to the
 * kernel by value.
 *
 * Rules, per (image b, phrase p):
 *   - valid: the phrase has a bit set among the tokens 0..T-1 and its clamped gt_count is > 0.  A phrase that is not valid takes
 *     part in nothing: its rows are padding (below) and valid = 0;
 *   - score of query q: the maximum of prob[b, q, t] over the tokens t of the phrase.  A NaN among them makes the score NaN (the
 *     canonical quiet NaN, 0x7FC00000); a zero maximum is +0.0;
 *   - ranking: the stable descending order of stable_desc.h (values descending, equal values by ascending query, NaN in front);
 *     the first kc = min(k_max, Q) queries are the candidates, rank 0 first;
 *   - candidate box: the detections tail's arithmetic (topk_select.h, box_to_output) with the output frame equal to the image
 *     frame (h, w), i.e. scale 1: x0 = fl(fl(cx - fl(0.5 w)) img_w), ..., clipped with fminf(fmaxf(x, 0), img_w) (a NaN coordinate
 *     therefore clips to 0); a candidate whose clipped box is empty stays a candidate and overlaps nothing;
 *   - ground truth: the first gt_count boxes; with merged != 0 they are first replaced by their ONE union box (fminf of the x0 and
 *     y0, fmaxf of the x1 and y1);
 *   - IoU in fp64, every operation rounded on its own (no contraction), all coordinates widened to fp64 first:
 *     da = (x1 - x0)(y1 - y0), ga likewise, w = fmin(x1, gx1) - fmax(x0, gx0), h likewise; iou = 0 where w <= 0 or h <= 0, else
 *     i = w h and iou = i / (da + ga - i) -- no `+ 1` -- and 0 where that quotient is a NaN.  top_iou is the maximum over the GTs;
 *   - hit: top_iou >= thr.  first_hit is the rank of the first candidate that hits, k_max where none does.
 *
 * Outputs, every element written exactly once: top_query [B, P, k_max] i32, -1 behind the kc candidates; top_score [B, P, k_max]
 * fp32 and top_iou [B, P, k_max] fp64, 0 behind them; first_hit [B, P, n_thr] i32; valid [B, P] u8.  The rows of a phrase that is
 * not valid are -1 / 0 / 0 / k_max.
 *
 * General contract (as zira_msda.h): device pointers to contiguous arrays, aligned to their element type; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream); the entry only enqueues ONE launch (one workgroup per (image,
 * phrase)), never synchronises, allocates nothing, needs no workspace and is capturable into a hipGraph; no global atomics: the
 * result depends on the inputs alone, two calls give the same bits.  Served: 1 <= B <= ZIRA_PHRASE_MAX_B, 1 <= Q <=
 * ZIRA_PHRASE_MAX_Q, 1 <= T <= ZIRA_PHRASE_MAX_T, 1 <= P <= ZIRA_PHRASE_MAX_P, 1 <= G <= ZIRA_PHRASE_MAX_G, 1 <= k_max <=
 * ZIRA_PHRASE_MAX_K, 1 <= n_thr <= ZIRA_PHRASE_MAX_THRS; anything else, or a null pointer, returns ZIRA_MSDA_EINVAL: host
 * arithmetic, nothing is launched.  Return 0, ZIRA_MSDA_EINVAL or a hipError_t cast to int.
 */
#ifndef ZIRA_PHRASE_H_
#define ZIRA_PHRASE_H_

#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h" /* ZIRA_MSDA_EINVAL */

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_PHRASE_MAX_B 65535
#define ZIRA_PHRASE_MAX_Q 1024
#define ZIRA_PHRASE_MAX_T 256
#define ZIRA_PHRASE_MAX_P 256
#define ZIRA_PHRASE_MAX_G 64
#define ZIRA_PHRASE_MAX_K 32
#define ZIRA_PHRASE_MAX_THRS 10

/* bytes of dynamic LDS the launch takes per block (host arithmetic); 0: a shape the kernel declines */
size_t zira_phrase_match_lds_bytes(int Q, int T, int G, int k_max, int n_thr);

int zira_phrase_match_f32(const float *prob, const float *boxes, const float *sizes, const uint32_t *phrase_bits,
                          const float *gt_boxes, const int32_t *gt_count, int B, int Q, int T, int P, int G, int k_max,
                          const double *iou_thrs, int n_thr, int merged, int32_t *top_query, float *top_score, double *top_iou,
                          int32_t *first_hit, unsigned char *valid, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_PHRASE_H_ */
