/*
 * zira_prompt.h -- C ABI of the prompt-tuning baseline's substitution (csrc/prompt.hip), a public header of libzira_msda.so
 * beside zira_msda.h.  Reference semantics: models/GroundingDINO/groundingdino_dt.py, forward (:521-531), as it runs when
 * `use_prompt_tuning` is on: the encoded text is cloned and, image by image and category by category, the rows a category's
 * token mask selects are overwritten with the category's entry of `prompt_memory_pool`.
 *
 * The loop is replaced by two index tables, built once per (captions, pool) on the host (prompt.py, build_table):
 *
 *   table [B, T, 2] int32: (segment, row) of the pool row that replaces x[b, t, :], or (-1, -1) where the row stays.  Where
 *     two categories of one image claim a token the later one is in the table, as the loop's order gives.
 *   segments [n_segments]: the pool entries, each a separate fp32 tensor [rows, D] (contiguous, 16-byte aligned), reached by
 *     pointer -- a device table as zira_optim_segment / zira_ema_segment, so the entries stay the separate parameters they are.
 *     The pool's rows are numbered segment after segment: r = (rows of the segments before) + row, n_rows of them.
 *   occ_start [n_rows + 1], occ [n_occ] int32: per pool row r the flat positions b * T + t that the table gives to it,
 *     ascending; CSR.
 *
 *   forward:   out[b, t, :] = table[b, t].segment < 0 ? x[b, t, :] : segments[segment].param[row, :]
 *   backward:  g_pool[r, :] = sum over occ[occ_start[r] .. occ_start[r + 1]) of grad_out[position, :], added in list order in
 *              fp32 (0 for an empty list); g_pool is ONE [n_rows, D] buffer, the entries' gradients are its row ranges;
 *              gx[b, t, :] = table[b, t].segment < 0 ? grad_out[b, t, :] : 0   (skipped when gx == NULL: without the language
 *              side branch x carries no gradient).
 *
 * Limits: 1 <= B <= ZIRA_PROMPT_MAX_B, 1 <= T <= ZIRA_PROMPT_MAX_T, D a multiple of 4 in 4 .. ZIRA_PROMPT_MAX_D,
 * 1 <= n_segments <= ZIRA_PROMPT_MAX_SEGMENTS, 1 <= n_rows <= ZIRA_PROMPT_MAX_ROWS, 0 <= n_occ <= B * T.
 * zira_prompt_supported answers 1 inside them and 0 outside; callers take the op chain there.
 *
 * General contract (as zira_clslinear.h):
 *   - device pointers to contiguous fp32 (tables: int32), x / out / grad_out / gx / g_pool and every segment 16-byte aligned:
 *     every access is a 16-byte vector load or store of a whole row quarter;
 *   - a table entry outside its segment (segment >= n_segments, row >= the segment's rows) is treated as -1 in the forward, an
 *     occurrence outside [0, B * T) is skipped in the backward: no table makes the kernels leave their buffers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); the entry points only enqueue, never synchronise,
 *     read nothing back to the host, allocate nothing and are capturable into a hipGraph;
 *   - no atomics: a pool row's gradient is summed by one wave in list order and stored once -- two calls on the same inputs give
 *     the same bits;
 *   - return value: 0, a hipError_t cast to int, or -1 for arguments the kernels decline (a null or misaligned pointer, a shape
 *     outside the limits): nothing is launched then.
 *
 * Launches: the forward is one, the backward is one.
 */
#ifndef ZIRA_PROMPT_H_
#define ZIRA_PROMPT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_PROMPT_MAX_B 64
#define ZIRA_PROMPT_MAX_T 256
#define ZIRA_PROMPT_MAX_D 4096
#define ZIRA_PROMPT_MAX_SEGMENTS 4096
#define ZIRA_PROMPT_MAX_ROWS 65536

typedef struct zira_prompt_segment {
    void *param;     /* the pool entry's data: fp32 [rows, D], contiguous, 16-byte aligned */
    int64_t rows;
} zira_prompt_segment;

int zira_prompt_supported(int B, int T, int D, int n_segments, long long n_rows);

int zira_prompt_substitute_fwd_f32(const float *x, const int32_t *table, const zira_prompt_segment *segments, int B, int T, int D,
                                   int n_segments, float *out, void *stream);

/* gx NULL: not computed */
int zira_prompt_substitute_bwd_f32(const float *grad_out, const int32_t *table, const int32_t *occ_start, const int32_t *occ,
                                   int B, int T, int D, long long n_rows, int n_occ, float *g_pool, float *gx, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_PROMPT_H_ */
