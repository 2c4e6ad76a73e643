/*
 * zira_clslinear.h -- C ABI of the trained class head of the linear-probing baseline (csrc/clslinear.hip), a public header of
 * libzira_msda.so beside zira_msda.h.  Reference semantics: models/GroundingDINO/utils.py, ContrastiveEmbedwithLinear (:272-310)
 * followed by recover_to_cls_logits (:312-320), as groundingdino_dual_zero_rep_branch.py builds and calls them when
 * `use_cls_linear` is on (:317-319, :549-552, :571-572).
 *
 * Shapes: x [R, 256] rows with R = S * B * Q (S stacked prediction sets, B images, Q queries; the image of row r is
 * b = (r / Q) % B), W [256, 256] (out, in) and bias [256] of `cls_linear`, text [B, T, 256] with T <= 256, text_token_mask
 * [B, T] (1 = a real token), cat_token_mask [B, Cmax, Tmax] uint8 with n_cat [B] and n_tok [B] as zira_cat_logits_fwd_f32
 * takes them (Cmax <= 256, Cmax and Tmax <= T_out), cat_token_range [B, Cmax, 2] int32 = the first set token of a category's
 * mask row and one past its last (0, 0 for an empty row): where the scan of a category starts and ends.
 *
 *     z        = W x + bias                                                   [R, 256]   (never leaves the chip)
 *     l[r, t]  = z[r] . text[b, t]   for t < min(n_tok[b], T) with text_token_mask[b, t], -inf elsewhere       (never stored)
 *     out[r, c] = max over the tokens t of category c (cat_token_mask[b, c, t]) of l[r, t],  argmax[r, c] = the FIRST such t
 *                 in token order (the rule of zira_cat_logits_fwd_f32; one definition, csrc/cat_max.h)         for c < n_cat[b]
 *     out[r, c] = for_fill, argmax[r, c] = -1   for c >= n_cat[b], for a category without tokens or with -inf logits only
 *   out is [R, T_out] (T_out = max_text_len), argmax [R, Cmax].
 *
 *   backward, from grad_out [R, T_out] (only columns c < n_cat[b] with argmax[r, c] >= 0 are read):
 *     gz[r, :] = sum_c grad_out[r, c] * text[b, argmax[r, c], :]             a category's gradient lands on exactly one token
 *     gx = gz W   (skipped when gx == NULL: under pure linear probing x carries no gradient);   g_w = gz^T x;   g_b = sum_r gz
 *
 * Arithmetic: plain fp32 MFMA with fp32 accumulation, as zira_adapter_fwd_f32: these weights are TRAINED, the split
 * arithmetics kept for frozen weights do not apply.
 *
 * General contract (as zira_adapter.h):
 *   - device pointers to contiguous fp32 (masks: uint8; counts, ranges, argmax: int32), x / w / bias / text / gx / g_w /
 *     g_b 16-byte aligned; `workspace` 16-byte aligned and of zira_cls_linear_workspace_floats(R, 256, T, Cmax) floats, no
 *     initialisation needed, not shared by calls that may run at the same time (only the backward uses it);
 *   - `counter` points to one uint32 that is 0 before the first call and is used by no two calls at the same time; the backward
 *     leaves it 0 again.  It counts the blocks that have stored their column sums of gz (an integer atomic); the last one adds
 *     them, kept in double, in index order;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no floating-point atomics anywhere: g_b as above, g_w through zira_xty_f32, whose partial tiles are folded in a fixed
 *     order too -- two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, a shape
 *     whose workspace function answers 0, R no multiple of B * Q, Cmax or Tmax above T_out): nothing is launched then.
 *
 * Launches: the forward is one.  The backward is one of its own (the rows' gz, g_b and, when asked for, gx) and the two of
 * zira_xty_f32 for g_w.
 */
#ifndef ZIRA_CLSLINEAR_H_
#define ZIRA_CLSLINEAR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* floats of workspace for the backward; 0: a shape the kernels decline (D != 256, T or Cmax outside 1..256, R < 1 or above 2^22) */
size_t zira_cls_linear_workspace_floats(long long R, int D, int T, int Cmax);

int zira_cls_linear_logits_fwd_f32(const float *x, const float *w, const float *bias, const float *text,
                                   const uint8_t *text_token_mask, const uint8_t *cat_token_mask, const int32_t *cat_token_range,
                                   const int32_t *n_cat, const int32_t *n_tok, long long R, int B, int Q, int T, int T_out,
                                   int Cmax, int Tmax, float for_fill, float *out, int32_t *argmax, void *stream);

/* gx NULL: not computed */
int zira_cls_linear_logits_bwd_f32(const float *grad_out, const int32_t *argmax, const int32_t *n_cat, const int32_t *n_tok,
                                   const float *x, const float *w, const float *text, long long R, int B, int Q, int T, int T_out,
                                   int Cmax, float *gx, float *g_w, float *g_b, float *workspace, uint32_t *counter,
                                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_CLSLINEAR_H_ */
