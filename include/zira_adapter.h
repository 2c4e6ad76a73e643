/*
 * zira_adapter.h -- C ABI of the gated bottleneck adapter (csrc/adapter.hip), a public header of libzira_msda.so beside
 * zira_msda.h.  Reference semantics: models/GroundingDINO/adapter.py, class Adapter (:124-179), as the deformable encoder and
 * decoder layers of transformer_for_adapter.py use it beside their FFN (:846-886, :965-1012) when `use_adapter` is on.
 *
 * Shapes: x [M, 256] rows, W_down [64, 256], b_down [64], W_up [256, 64], b_up [256], gate [G, 256] with 1 <= G <= 8, or
 * gate = NULL and G = 0 for `use_gate = False`.
 *
 *     h     = relu(W_down x + b_down)                                  [M, 64]
 *     cos_g = (x . gate_g) / (|x| |gate_g|);  amax = the FIRST g with the largest cos_g (torch.max);  cos = cos_amax
 *     scale = gate_base_scale * sigmoid(gate_T * cos)                  per row;  the constant gate_base_scale when G = 0
 *     y     = (W_up h + b_up) * scale                                  [M, 256]
 *     loss  = mean|x| when self_kd != 0 (the reference takes the L1 of the INPUT, adapter.py:177), else 0
 *   A row of zero norm gives NaN in cos, scale and y, as the reference's division does; nothing special-cases it.
 *
 *   backward, from grad_y [M, 256] and grad_loss (one float, NULL = 0):
 *     gu = grad_y * scale;  g_W_up = gu^T h;  g_b_up = sum_rows gu
 *     gh = (W_up^T gu) o [h > 0];  g_W_down = gh^T x;  g_b_down = sum_rows gh
 *     g_cos = (grad_y . (W_up h + b_up)) * gate_T * scale * (1 - scale / gate_base_scale)
 *     gx = W_down^T gh + g_cos * (ghat_amax - cos * xhat) / |x| + sign(x) * grad_loss / (256 M)      (sign(0) = 0)
 *     g_gate[amax] += g_cos * (xhat - cos * ghat_amax) / |gate_amax|;  the other gate rows receive nothing from the row
 *
 * Arithmetic: plain fp32 MFMA with fp32 accumulation, as zira_rowgemm_f32.  These weights are TRAINED (they change every step
 * and their gradients are wanted), so the split arithmetics kept for frozen weights (f16x2, bf16x3: packed or split once, reused
 * for a whole task) do not apply here.  Divisions and roots are the correctly rounded ones.
 *
 * General contract (as zira_msda.h):
 *   - device pointers to contiguous fp32 (amax: int32), 16-byte aligned; `workspace` 16-byte aligned and of
 *     zira_adapter_workspace_floats(M) floats, no initialisation needed, not shared by calls that may run at the same time;
 *   - `counter` points to one uint32 that is 0 before the first call and is used by no two calls at the same time; the forward
 *     leaves it 0 again.  It counts the blocks that have stored their partial of sum|x| (an integer atomic); the last one adds
 *     the partials, kept in double, in index order.  Unused (may be NULL) when self_kd == 0;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no floating-point atomics anywhere: the sums over the M rows (g_b_up, g_b_down, g_gate) are carried per block of 128 rows
 *     and folded from double partials in index order, and the two weight products run through zira_xty_f32, whose partial tiles
 *     are folded in a fixed order too -- two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, G outside
 *     0..8, a row count whose workspace function answers 0): nothing is launched then.
 *
 * Launches: the forward is one.  The backward is two of its own (the row pass: grad_y -> gh, gx and the per-block sums; the
 * fold of those sums) and the two tall-reduction products of zira_xty_f32 (two launches each).
 */
#ifndef ZIRA_ADAPTER_H_
#define ZIRA_ADAPTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* floats of workspace for either direction; 0: a shape the kernels decline (D != 256, H != 64, M < 1 or M above 2^22) */
size_t zira_adapter_workspace_floats(long long M, int D, int H);

/* writes y [M, 256], loss [1] and, for the backward, h [M, 64], scale [M], amax [M], cosv [M], rnorm [M] (1 / |x|) */
int zira_adapter_fwd_f32(const float *x, const float *w_down, const float *b_down, const float *w_up, const float *b_up,
                         const float *gate, long long M, int G, float gate_T, float gate_base_scale, int self_kd, float *y,
                         float *loss, float *h, float *scale, int32_t *amax, float *cosv, float *rnorm, float *workspace,
                         uint32_t *counter, void *stream);

/* g_gate [G, 256] (NULL when G = 0); grad_loss NULL = 0 */
int zira_adapter_bwd_f32(const float *grad_y, const float *grad_loss, const float *x, const float *h, const float *scale,
                         const int32_t *amax, const float *cosv, const float *rnorm, const float *w_down, const float *w_up,
                         const float *b_up, const float *gate, long long M, int G, float gate_T, float gate_base_scale,
                         int self_kd, float *gx, float *g_w_down, float *g_b_down, float *g_w_up, float *g_b_up, float *g_gate,
                         float *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_ADAPTER_H_ */
