/*
 * zira_lora.h -- C ABI of the low-rank language side branch (csrc/lora.hip), a public header of libzira_msda.so beside zira_cet.h.
 * Reference semantics: `RepZeroLoRA.forward` in training mode (models/GroundingDINO/adapter.py:227-259), the low-rank form of
 * the language side branch beside `feat_map`.
 *
 * Shapes: x [M, E] rows of encoder states, W_down [R, E], W_up [256, R], W_twin [256, E] (`freeze_linear`), scaling [1].  No
 * biases.  Limits: E a multiple of 32 up to ZIRA_LORA_MAX_E, R a multiple of 32 up to ZIRA_LORA_MAX_R, the output width is
 * ZIRA_LORA_OUT, 1 <= M <= ZIRA_LORA_MAX_ROWS.
 *
 *     h      = x W_down^T                                              [M, R]
 *     branch = scaling * (h W_up^T)                                    [M, 256]
 *     out    = branch + x W_twin^T                                     [M, 256]
 *     loss   = mean(sl1(branch)) + mean(sl1(out)) over all M * 256 elements each; sl1 is SmoothL1 to zero with beta = 1:
 *              v^2 / 2 below 1, |v| - 1/2 from there on
 *
 *   backward, from grad_out [M, 256] (NULL = zeros) and grad_loss (one float on the device, NULL = 0), s = grad_loss / (256 M),
 *   sl1'(v) = v below 1, sign(v) from there on:
 *     gt = grad_out + s * sl1'(out)                                    (the gradient of x W_twin^T)
 *     gp = gt + s * sl1'(branch)                                       (the gradient of branch)
 *     g_scaling = sum over all elements of gp * (h W_up^T);   gb = scaling * gp
 *     g_h = gb W_up;  g_W_up = gb^T h;  g_W_down = g_h^T x;  g_W_twin = gt^T x
 *     gx = g_h W_down + gt W_twin                                      (only when gx != NULL)
 *
 * What the forward keeps for the backward: `out` and `h`.  branch is formed again as scaling * (h W_up^T) by the instructions
 * that formed it in the forward, from the h they read: the same bits, so sl1' takes the arm the loss summed.  Keeping branch
 * instead would save the backward R / 32 short chains a tile and cost M * 256 floats; h is needed by g_W_up in any case.
 *
 * Arithmetic: plain fp32 MFMA (v_mfma_f32_32x32x2_f32) with fp32 accumulation.  All three weights are TRAINED, so the split
 * arithmetics kept for frozen weights do not apply.
 *
 * Forward, ONE launch.  A wave (a block of its own) owns 32 rows and a share of the in_features: zira_lora_splits(M, E) = S waves
 * share a row tile (S = 1 when the row tiles alone fill the chip).  With per = ceil((E / 32) / S), wave (tile, s) takes the
 * panels of 32 features s * per ... s * per + per - 1 (the last wave's share may be shorter): it reads its panel of x ONCE and
 * feeds it to h^T = W_down x^T and to twin^T = W_twin x^T, whose accumulators stay in registers.  With S > 1 each wave stores its
 * partial h and twin and draws the tile's integer ticket; the wave that draws the last one adds the S partials IN INDEX ORDER
 * (its own from memory too; in double, rounded once).  h^T is then the operand of out^T = W_up h^T as it stands -- the down
 * product is taken transposed, so the hidden activation reaches the second product without LDS; the same wave stores h, forms
 * branch and out, stores out and leaves the tile's two SmoothL1 sums as doubles; the wave that draws the last ticket of the
 * tiles adds those doubles in index order.  Both tickets wrap to zero, so a captured launch replays without a memset node.
 *
 * Backward: an element pass dealt by (row tile, 32 output columns) (branch again, gt, gb, the wave's part of g_scaling as a
 * double -- one number out of 256 M products that cancel, so its terms are taken in double: h W_up^T once more with plain
 * double FMAs, times the element's gradient before rounding), g_h = gb W_up by (row tile, 32 hidden units), one fold of the
 * doubles in index order, zira_xty_f32 for the three weight gradients (two launches each) and, only when gx != NULL, gx by
 * (row tile, 32 features).
 *
 * General contract (as zira_cet.h):
 *   - device pointers to contiguous fp32, 16-byte aligned;
 *   - `tickets`: zira_lora_ticket_words(M) uint32, ZERO before the first call; every forward leaves them zero again.
 *     `workspace`: zira_lora_fwd_workspace_floats / zira_lora_bwd_workspace_floats floats, no initialisation needed.  Neither is
 *     shared by calls that may run at the same time;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no floating-point atomics anywhere and every sum in a fixed order: two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, a shape
 *     outside the limits): nothing is launched then.
 */
#ifndef ZIRA_LORA_H_
#define ZIRA_LORA_H_

#include <stddef.h>
#include <stdint.h>

#define ZIRA_LORA_MAX_E 1024
#define ZIRA_LORA_MAX_R 256
#define ZIRA_LORA_OUT 256
#define ZIRA_LORA_MAX_ROWS 16384

#ifdef __cplusplus
extern "C" {
#endif

/* 1 inside the limits above, 0 outside */
int zira_lora_supported(long long M, int E, int R);

/* waves that share a row tile of 32 rows (a function of M and E alone); 0 outside the limits */
int zira_lora_splits(long long M, int E);

size_t zira_lora_ticket_words(long long M);

size_t zira_lora_fwd_workspace_floats(long long M, int E, int R);

size_t zira_lora_bwd_workspace_floats(long long M, int E, int R);

/* writes out [M, 256], loss [1] and h [M, R] */
int zira_lora_fwd_f32(const float *x, const float *w_down, const float *w_up, const float *w_twin, const float *scaling,
                      long long M, int E, int R, float *out, float *loss, float *h, float *workspace, uint32_t *tickets,
                      void *stream);

/* gx NULL: not computed.  gb, gt [M, 256] and gh [M, R] are the caller's buffers, written here */
int zira_lora_bwd_f32(const float *grad_out, const float *grad_loss, const float *x, const float *out, const float *h,
                      const float *w_down, const float *w_up, const float *w_twin, const float *scaling, long long M, int E,
                      int R, float *gb, float *gt, float *gh, float *gx, float *g_w_down, float *g_w_up, float *g_w_twin,
                      float *g_scaling, float *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_LORA_H_ */
