/*
 * zira_prompt_memory.h -- C ABI of the text-memory replay's loss (csrc/prompt_memory.hip), a public header of libzira_msda.so
 * beside zira_prompt.h.  Reference semantics: models/GroundingDINO/groundingdino_dt.py, forward (:509-519) and replay_memory
 * (:824-834), as they run when `use_prompt_memory` is on: the encoded text is cloned, image by image and category by category the
 * rows a learned category's token mask selects are overwritten with the category's entry of `prompt_memory_pool`, and
 * `L1Loss(mean)(target, encoded_text)` pulls the text back to what was stored.
 *
 * The loop is replaced by the index tables of zira_prompt.h, unchanged (prompt.py, build_table): table [B, T, 2] int32 of
 * (segment, row) or (-1, -1), the device table of zira_prompt_segment pointers to the pool entries (each a separate fp32 [rows, D]
 * tensor; passed here as `const void *segments`, the address of that device table), and the CSR occurrence list
 * occ_start [n_rows + 1] / occ [n_occ] of flat positions b * T + t per pool row.  With N = B * T * D and pool(b, t) the row the
 * table names:
 *
 *   forward:   loss = (float)((1 / N) * sum over substituted (b, t), over d, of |pool(b, t)[d] - x[b, t, d]|).  The difference and
 *              the absolute value are fp32, as ATen takes them; the sum is carried in double: a wave per token row, one double per
 *              block in the workspace, and the last block to arrive adds the blocks' doubles in index order.  Unsubstituted rows
 *              have target == x and add nothing.
 *   backward:  s = g * (1 / N) in fp32 -- ATen's `grad / numel` on the device, a product with the reciprocal --, g read from the
 *              device by pointer;
 *              gx[b, t, d]  = -sign(pool - x) * s on substituted rows, 0 elsewhere (sign(0) = 0)   (skipped when gx == NULL);
 *              g_pool[r, d] = sum over occ[occ_start[r] .. occ_start[r + 1]) of +sign(pool[r, d] - x[position, d]) * s, added in
 *              list order in fp32 (0 for an empty list); g_pool is ONE [n_rows, D] buffer, the entries' gradients are its row
 *              ranges (skipped when g_pool == NULL: the entries are memory, not parameters).
 *
 * Limits: those of zira_prompt.h (ZIRA_PROMPT_MAX_B, _T, _D, _SEGMENTS, _ROWS; D a multiple of 4), 0 <= n_occ <= B * T.
 * zira_pmem_supported answers 1 inside them and 0 outside; callers take the op chain there.
 *
 * Workspace: zira_pmem_workspace_bytes(B, T) bytes (0 outside the limits), 16-byte aligned.  Its first word is the arrival
 * ticket: ZERO before the first call, and every forward leaves it at zero again -- the last block to arrive wraps it --, so a
 * captured launch replays with no memset node.  Behind the first 16 bytes lie the blocks' doubles, which need no initial value.
 * One workspace serves one stream at a time.
 *
 * General contract (as zira_prompt.h):
 *   - device pointers to contiguous fp32 (tables: int32), x / gx / g_pool and every segment 16-byte aligned: every access to them
 *     is a 16-byte vector load or store of a whole row quarter;
 *   - a table entry outside its segment (segment >= n_segments, row >= the segment's rows) counts as -1, an occurrence outside
 *     [0, B * T) or at a position whose table entry counts as -1 is skipped: no table makes the kernels leave their buffers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no float atomics (the ticket is an integer): two calls on the same inputs give the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, a shape
 *     outside the limits): nothing is launched then.
 *
 * Launches: the forward is one, the backward is one (none when both gx and g_pool are NULL).
 */
#ifndef ZIRA_PROMPT_MEMORY_H_
#define ZIRA_PROMPT_MEMORY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int zira_pmem_supported(int B, int T, int D, int n_segments, long long n_rows);

size_t zira_pmem_workspace_bytes(int B, int T);

int zira_pmem_loss_fwd_f32(const float *x, const int32_t *table, const void *segments, int B, int T, int D,
                           int n_segments, float *loss, void *workspace, void *stream);

/* gx NULL / g_pool NULL: not computed */
int zira_pmem_loss_bwd_f32(const float *grad_loss, const float *x, const int32_t *table, const void *segments,
                           const int32_t *occ_start, const int32_t *occ, int B, int T, int D, int n_segments, long long n_rows,
                           int n_occ, float *g_pool, float *gx, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_PROMPT_MEMORY_H_ */
