/*
 * zira_rsb_ml.h -- C ABI of the fused epilogue of the multilayer-branch ZiRa side branches (csrc/rsb_ml.hip), a public
 * header of libzira_msda.so beside zira_msda.h.  Reference semantics: models/GroundingDINO/
 * groundingdino_dual_zero_rep_multilayer_branch.py, RepZeroLinear.forward (:116-146) and RepZeroConv2dGN.forward (:69-113),
 * training mode.  The two dense contractions y_branch = F(x; W, b) and y_twin = F(x; W_f, b_f) stay with the caller's GEMM
 * library; everything after them is here.
 *
 * General contract (as zira_msda.h):
 *   - device pointers to contiguous fp32; the [n] / [B, C, HW] tensors 16-byte aligned, `workspace` 8-byte aligned and of
 *     the size its function names (no initialisation needed); `scaling`, `loss`, `g_scaling`, `grad_loss` point to one float;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never
 *     synchronise, allocate nothing and are capturable into a hipGraph;
 *   - no floating-point atomics and no arrival counters: per-block partial sums go to the workspace in double and are
 *     combined in a fixed order, so two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer,
 *     C % G != 0, a size whose workspace function answers 0): nothing is launched then.
 *
 * Language branch (RepZeroLinear), n elements:
 *     branch = scaling * y_branch;  out = branch + y_twin;  loss = mean|branch| + mean|out|
 *   backward, grad_out (d/dout, NULL = zeros) and grad_loss (d/dloss, NULL = 0):
 *     d_out = grad_out + grad_loss * sign(out) / n;  d = d_out + grad_loss * sign(branch) / n
 *     g_twin = d_out;  g_branch = scaling * d;  g_scaling = sum(y_branch * d);  sign(0) = 0
 *   One launch and one one-block finishing launch each way.
 *
 * Vision branch (RepZeroConv2dGN), [B, C, HW] with G groups, N = B * C * HW:
 *     x = scaling * y_branch + y_twin;  out = gamma_c * (x - mean_g) * rstd_g + beta_c   (biased variance, eps inside the root)
 *     loss = mean|scaling * y_branch| + mean|out|;   mean / rstd [B * G] are written for the backward
 *   backward (`out` is the forward's output):
 *     dout = grad_out + grad_loss * sign(out) / N;  g_gamma_c = sum_{b,hw} dout * xhat;  g_beta_c = sum_{b,hw} dout
 *     dx = rstd * (dout * gamma - mean_group(dout * gamma) - xhat * mean_group(dout * gamma * xhat))
 *     d = dx + grad_loss * sign(scaling * y_branch) / N;  g_branch = scaling * d;  g_scaling = sum(y_branch * d)
 *     g_twin = dx, skipped when g_twin is NULL.
 *   Two launches over the tensor (statistics or sums per block, then the element pass) and one small finishing launch
 *   each way.  The variance is formed from values centred on each block's own mean and joined exactly in double.
 */
#ifndef ZIRA_RSB_ML_H_
#define ZIRA_RSB_ML_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* floats of workspace for both directions; 0: a size the kernels decline (n == 0) */
size_t zira_rsb_l1_workspace_floats(size_t n);

int zira_rsb_l1_fwd_f32(const float *y_branch, const float *y_twin, const float *scaling, size_t n, float *out, float *loss,
                        float *workspace, void *stream);

int zira_rsb_l1_bwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *grad_out,
                        const float *grad_loss, size_t n, float *g_branch, float *g_twin, float *g_scaling, float *workspace,
                        void *stream);

/* floats of workspace for both directions; 0: a shape the kernels decline (a non-positive size, C % G != 0, B * C above
 * 2^20 or HW above 2^28) */
size_t zira_rsb_gn_workspace_floats(int B, int C, int HW, int G);

int zira_rsb_gn_fwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *gamma, const float *beta,
                        int B, int C, int HW, int G, float eps, float *out, float *loss, float *mean, float *rstd,
                        float *workspace, void *stream);

int zira_rsb_gn_bwd_f32(const float *y_branch, const float *y_twin, const float *scaling, const float *gamma, const float *mean,
                        const float *rstd, const float *out, const float *grad_out, const float *grad_loss, int B, int C, int HW,
                        int G, float *g_branch, float *g_twin, float *g_scaling, float *g_gamma, float *g_beta, float *workspace,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_RSB_ML_H_ */
