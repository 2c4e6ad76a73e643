/*
 * zira_cet.h -- C ABI of the CET text adapter (csrc/cet.hip), a public header of libzira_msda.so beside zira_adapter.h.
 * Reference semantics: models/GroundingDINO/groundingdino_dt.py (:182-215, :499-507) with `use_cet` and cet_type = "Adapter": the
 * gated bottleneck `Adapter` of adapter.py:124-179 beside `feat_map`, from the text encoder's states to the projected text, and
 * the zero-interference term on its output.
 *
 * Shapes: x [M, E] rows of encoder states, W_down [H, E], b_down [H], W_up [256, H], b_up [256], gate [G, E] with 1 <= G <= 8 (or
 * gate = NULL and G = 0 for `use_gate = False`), feat [M, 256] (feat_map's output).  Limits: E a multiple of 32 up to
 * ZIRA_CET_MAX_E, H a multiple of 32 up to ZIRA_CET_MAX_H, the output width is ZIRA_CET_OUT, 1 <= M <= ZIRA_CET_MAX_ROWS.
 *
 *     h     = relu(W_down x + b_down)                                  [M, H]      (never stored by the forward)
 *     cos_g = (x . gate_g) / (|x| |gate_g|);  amax = the FIRST g with the largest cos_g (torch.max);  cos = cos_amax
 *     scale = gate_base_scale * sigmoid(gate_T * cos)                  per row;  the constant gate_base_scale when G = 0
 *     out   = (W_up h + b_up) * scale                                  [M, 256]
 *     enc   = feat + out                                               [M, 256]
 *     loss  = mean over all M * 256 elements of L(out), L chosen by loss_type: ZIRA_CET_LOSS_NONE (loss = 0), _L1 |o|,
 *             _L2 o^2, _SMOOTH_L1 (beta = 1: o^2 / 2 below 1, |o| - 1/2 from there on)
 *   A row of zero norm gives NaN in cos, scale, out and enc, as the reference's division does; nothing special-cases it.
 *
 *   backward, from grad_enc [M, 256] (NULL = zeros) and grad_loss (one float on the device, NULL = 0), s = grad_loss / (256 M):
 *     g_out = grad_enc + L'(out) * s          (L1: sign, sign(0) = 0;  L2: 2 o;  smooth L1: o below 1, sign from there on)
 *     g_feat = grad_enc as it stands: the caller hands it on, no kernel touches it
 *     gu = g_out * scale;  g_W_up = gu^T h;  g_b_up = sum_rows gu
 *     gh = (gu W_up) o [h > 0];  g_W_down = gh^T x;  g_b_down = sum_rows gh
 *     g_cos = (g_out . out / scale) * gate_T * scale * (1 - scale / gate_base_scale)
 *     gx = gh W_down + g_cos * (ghat_amax - cos * xhat) / |x|                                   (only when gx != NULL)
 *     g_gate[amax] += g_cos * (xhat - cos * ghat_amax) / |gate_amax|;  the other gate rows receive nothing from the row
 *
 * What the forward keeps for the backward: `out` and the row's gate (scale, amax, cos, 1 / |x|) -- BOTH, because each alone
 * costs more than it saves.  The loss's derivative needs out itself (its sign or value, bit for bit what the loss summed), and
 * g_cos needs W_up h + b_up, which is out / scale: without `out` the backward would run the up product a second time.  The
 * gate is four numbers a row; without it the backward would repeat the row pass over x and could choose another arg-max than
 * the forward on a near tie.  `h` is NOT kept (H = 1024 makes it four times `out`): the backward runs the down product again
 * and writes h then, because the weight gradient's tall product reads it from memory anyway.
 *
 * Arithmetic: plain fp32 MFMA (v_mfma_f32_32x32x2_f32) with fp32 accumulation.  These weights are TRAINED, so the split
 * arithmetics kept for frozen weights do not apply.  Divisions and roots are the correctly rounded ones.
 *
 * Forward, ONE launch.  A wave owns 32 rows and a share of the hidden units: zira_cet_splits(M, H) = S waves share a row tile
 * (S = 1 when the row tiles alone fill the chip).  Wave (tile, s) takes the panels of 32 hidden units p = s, s + S, ...: down
 * product over E, bias, ReLU, and at once the panel's part of the up product, whose 32 x 256 accumulators stay in registers.
 * With S > 1 each wave stores its partial accumulators and draws the tile's integer ticket; the wave that draws the last one
 * adds the S partials IN INDEX ORDER (its own from memory too), adds b_up, scales, adds feat, stores out and enc, and leaves the
 * tile's sum of L(out) as one double; the wave that draws the last ticket of the tiles adds those doubles in index order.  Both
 * tickets wrap to zero, so a captured launch replays without a memset node.
 *
 * Backward: a row pass (g_out, gu, the gate's coefficients, the gate's part of gx, g_b_up and g_gate per tile), a hidden pass
 * with the forward's split (h again, gh, g_b_down per tile), one fold of the tiles' doubles in index order, zira_xty_f32 for the
 * two weight gradients (two launches each) and, only when gx != NULL, gx += gh W_down.
 *
 * General contract (as zira_adapter.h):
 *   - device pointers to contiguous fp32 (amax: int32), 16-byte aligned;
 *   - `tickets`: zira_cet_ticket_words(M) uint32, ZERO before the first call; every forward leaves them zero again.  `workspace`:
 *     zira_cet_fwd_workspace_floats / zira_cet_bwd_workspace_floats floats, no initialisation needed.  Neither is shared by calls
 *     that may run at the same time;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no floating-point atomics anywhere and every sum in a fixed order: two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, a shape
 *     outside the limits): nothing is launched then.
 */
#ifndef ZIRA_CET_H_
#define ZIRA_CET_H_

#include <stddef.h>
#include <stdint.h>

#define ZIRA_CET_MAX_E 768
#define ZIRA_CET_MAX_H 1024
#define ZIRA_CET_OUT 256
#define ZIRA_CET_MAX_GATES 8
#define ZIRA_CET_MAX_ROWS 16384
#define ZIRA_CET_LOSS_NONE 0
#define ZIRA_CET_LOSS_L1 1
#define ZIRA_CET_LOSS_L2 2
#define ZIRA_CET_LOSS_SMOOTH_L1 3

#ifdef __cplusplus
extern "C" {
#endif

/* 1 inside the limits above, 0 outside */
int zira_cet_supported(long long M, int E, int H, int G);

/* waves that share a row tile of 32 rows (a function of M and H alone); 0 outside the limits */
int zira_cet_splits(long long M, int H);

size_t zira_cet_ticket_words(long long M);

size_t zira_cet_fwd_workspace_floats(long long M, int H);

size_t zira_cet_bwd_workspace_floats(long long M, int E, int H, int G);

/* writes enc [M, 256], loss [1] and, for the backward, out [M, 256], scale [M], amax [M], cosv [M], rnorm [M] (1 / |x|) */
int zira_cet_fwd_f32(const float *x, const float *feat, const float *w_down, const float *b_down, const float *w_up,
                     const float *b_up, const float *gate, long long M, int E, int H, int G, float gate_T,
                     float gate_base_scale, int loss_type, float *enc, float *loss, float *out, float *scale, int32_t *amax,
                     float *cosv, float *rnorm, float *workspace, uint32_t *tickets, void *stream);

/* gx NULL: not computed.  g_gate [G, E] (NULL when G = 0).  h, gh [M, H] and gu [M, 256] are the caller's buffers, written here */
int zira_cet_bwd_f32(const float *grad_enc, const float *grad_loss, const float *x, const float *out, const float *scale,
                     const int32_t *amax, const float *cosv, const float *rnorm, const float *w_down, const float *b_down,
                     const float *w_up, const float *gate, long long M, int E, int H, int G, float gate_T,
                     float gate_base_scale, int loss_type, float *h, float *gh, float *gu, float *gx, float *g_w_down,
                     float *g_b_down, float *g_w_up, float *g_b_up, float *g_gate, float *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_CET_H_ */
