/*
 * zira_vocab.h -- C ABI of the merged detections tail of a chunked vocabulary (csrc/vocab.hip), a public header of
 * libzira_msda.so beside zira_msda.h.  A category list that tokenises longer than the model's max_text_len is run in J chunks;
 * each chunk leaves its own top-k candidates (zira_topk_rows_f32 over its [Q x C_j] probabilities), its own boxes and its own
 * label numbering.  This entry keeps the global top-k over all chunks and applies the evaluation tail of zira_detections_f32.
 *
 * Per image b, over the N = chunks->n candidate positions of its row:
 *   - the first min(k, N) positions of the stable descending order of cand_scores[b, :] are taken (csrc/stable_desc.h: equal
 *     scores by ascending position, -0.0 == +0.0, NaN first).  Every position counts, the padding of a short chunk included:
 *     the caller gives padding a score below every real candidate;
 *   - position p lies in chunk j = the last one with start[j] <= p;  index = cand_index[b, p] (a flat index into that
 *     chunk's [Q, classes[j]] tensor, 0 <= index < Q * classes[j]);  q = index / classes[j];
 *     label = label_offset[j] + index % classes[j];  box = boxes[j, b, q] (cxcywh in 0..1);
 *   - the box goes to pixels of the output size, is clipped, empty boxes are dropped and the rest compacted, with exactly the
 *     arithmetic of zira_detections_f32 (one definition, csrc/topk_select.h).
 * An index outside its chunk's range never makes the kernel read outside `boxes` (q is clamped); the row it yields is
 * unspecified.
 *
 * General contract (as zira_msda.h):
 *   - device pointers to contiguous arrays: cand_scores [B, N] fp32, cand_index [B, N] int64 (8-byte aligned), boxes
 *     [J, B, Q, 4] fp32 (16-byte aligned), sizes [B, 4] fp32 = (img_h, img_w, out_h, out_w);  outputs scores [B, k] fp32,
 *     labels [B, k] int64, xyxy [B, k, 4] fp32 (16-byte aligned), n_keep [B] int32: every element written once, zero at and
 *     behind n_keep[b];
 *   - `chunks` is a HOST descriptor, read during the call and handed to the kernel by value: nothing is uploaded;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry only enqueues ONE launch, never
 *     synchronises, allocates nothing, needs no workspace and is capturable into a hipGraph;
 *   - no global atomics: the result is a function of the input alone, two calls give the same bits;
 *   - return value: 0, ZIRA_MSDA_EINVAL (a null or misaligned pointer, B outside 1 .. ZIRA_VOCAB_MAX_B, J outside
 *     1 .. ZIRA_VOCAB_MAX_CHUNKS, N outside 1 .. ZIRA_VOCAB_MAX_CANDIDATES, k outside 1 .. ZIRA_VOCAB_MAX_K, Q < 1,
 *     start[0] != 0, starts not strictly ascending below N, classes[j] < 1, label_offset[j] < 0, Q * classes[j] or
 *     label_offset[j] + classes[j] above 2^31 - 1: host arithmetic, nothing is launched) or a hipError_t cast to int.
 */
#ifndef ZIRA_VOCAB_H_
#define ZIRA_VOCAB_H_

#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h" /* ZIRA_MSDA_EINVAL */

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_VOCAB_MAX_CHUNKS 64
#define ZIRA_VOCAB_MAX_CANDIDATES 16384
#define ZIRA_VOCAB_MAX_K 1024
#define ZIRA_VOCAB_MAX_B 65535

/* the chunk table: J chunks over n candidate positions; chunk j owns positions start[j] .. start[j + 1] - 1 (the last one
 * up to n - 1), has classes[j] categories and numbers them from label_offset[j] */
typedef struct zira_vocab_chunks {
    int32_t J, n;
    int32_t start[ZIRA_VOCAB_MAX_CHUNKS];
    int32_t classes[ZIRA_VOCAB_MAX_CHUNKS];
    int32_t label_offset[ZIRA_VOCAB_MAX_CHUNKS];
} zira_vocab_chunks;

/* bytes of LDS the launch for n candidate positions takes per block (host arithmetic); 0: an n the kernel declines */
size_t zira_det_merge_lds_bytes(int n);

int zira_det_merge_f32(const float *cand_scores, const int64_t *cand_index, const zira_vocab_chunks *chunks, const float *boxes,
                       int B, int Q, int k, const float *sizes, float *scores, int64_t *labels, float *xyxy, int32_t *n_keep,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_VOCAB_H_ */
