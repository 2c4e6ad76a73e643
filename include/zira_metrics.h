/*
 * zira_metrics.h -- C ABI of the device-side training metrics log (csrc/metrics.hip), the second public header of
 * libzira_msda.so beside zira_msda.h.  It replaces the bookkeeping the reference's trainer does on the host in every
 * iteration (detectron2 SimpleTrainer._write_metrics: `.cpu().item()` of every loss, np.mean over ranks, sum(), np.isfinite,
 * EventStorage histories read as np.median over the last 20 values by CommonMetricPrinter / JSONWriter).
 *
 * The log is a ring of fp32 rows in device memory, one row per iteration and one column per scalar, with a device cursor
 * (the number of rows ever recorded, int64) and a device first_bad (the cursor of the first row whose loss columns held an
 * inf or a NaN, -1 while there was none, int64).  The caller allocates all three and sets cursor = 0, first_bad = -1.
 *
 * General contract (as zira_msda.h):
 *   - device pointers unless a parameter says HOST; contiguous, row-major; fp32 sources and ring 4-byte aligned, int64 and
 *     fp64 arrays 8-byte aligned;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); both entry points only enqueue, never
 *     synchronise, allocate nothing, use no workspace, no global atomics, and are capturable into a hipGraph -- a captured
 *     zira_metrics_record_f32 re-reads its sources, the cursor and first_bad at every replay;
 *   - return value: 0, ZIRA_MSDA_EINVAL (a null or misaligned pointer, a count outside its range: nothing is launched and no
 *     memory is touched) or a hipError_t cast to int; never throws, never prints.
 *
 * zira_metrics_record_f32 appends one row:  ONE launch of one workgroup of one wave.
 *   sources (HOST, read during the call and copied into the kernel's arguments): the row's columns in order, first the n_dev
 *   device scalars src[0 .. n_dev) (each a pointer to one fp32: the loss tensors, the gradient norm, the found-inf flag, the
 *   loss scale), then the n_host floats host[0 .. n_host) by value (learning rate, data time, ...).
 *   cols = n_dev + n_host, 1 <= cols <= ZIRA_METRICS_MAX_COLS, 0 <= n_dev, 0 <= n_host <= ZIRA_METRICS_MAX_HOST.  The first
 *   n_loss columns (0 <= n_loss <= cols) are the losses.
 *   Lane c stores column c to ring[(cursor % rows) * cols + c] (bit patterns are copied; no arithmetic touches them).  If
 *   first_bad is -1 and a loss column of this row is an inf or a NaN, first_bad becomes cursor; once set it stays.  cursor is
 *   incremented last.  1 <= rows <= ZIRA_METRICS_MAX_ROWS.  Launches on one stream are ordered, which is all the kernel relies on.
 *
 * zira_metrics_window_f64 reduces the last n = min(window, cursor) rows:  ONE launch of cols + 1 workgroups of one wave.
 *   rings: `ranks` rings of [rows, cols] fp32, ring r starting at rings + r * rank_stride (elements; rank_stride >=
 *   rows * cols, ignored for ranks == 1), every rank's ring written under the same cursor (ranks above 1 come from an
 *   all-gather).  1 <= ranks <= ZIRA_METRICS_MAX_RANKS, 1 <= window <= ZIRA_METRICS_MAX_WINDOW, window <= rows.
 *   Per row and column, in fp64:  x = np.mean over ranks of the column's values -- numpy's order for a list of that length:
 *   the sum starts from -0.0 and runs left to right below 8 ranks; at 8 ranks it is ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
 *   (r6 + r7)); then 0.0 + that sum, then / ranks.  Column max_col (-1: none, else n_loss <= max_col < cols; the
 *   reference's data_time) takes np.max over ranks instead (a NaN wins).  The row's total_loss is 0.0 + x[0] + x[1] + ... + x[n_loss - 1], left to right (Python's
 *   sum(metrics_dict.values())), and is column `cols` of the result.
 *   out [3, cols + 1] fp64, every element written exactly once, rows oldest to latest:
 *     out[0][c] = x of the latest row;
 *     out[1][c] = np.median of the n values: np.mean of the middle one of the sorted values (0.0 + a, so a -0.0 comes out as
 *                 +0.0) or of the two middle ones for an even n ((0.0 + (a + b)) / 2); a NaN if any value is a NaN;
 *     out[2][c] = np.mean of the n values in numpy's order for a contiguous fp64 array of n <= 64 elements: below 8 as above;
 *                 from 8 on eight running sums r[j] = v[j] + v[8 + j] + v[16 + j] + ... over the whole groups of 8, combined
 *                 as above, the n % 8 leftover values added one by one, then 0.0 + that, then / n.
 *   With cursor == 0 every element is a NaN.
 *   Not promised: the sign and payload of a NaN result (they differ between processors).  Everything else is numpy's
 *   result bit for bit; the file is compiled with floating-point contraction off.
 */
#ifndef ZIRA_METRICS_H_
#define ZIRA_METRICS_H_

#include <stddef.h>
#include <stdint.h>

#include "zira_msda.h" /* ZIRA_MSDA_EINVAL */

#ifdef __cplusplus
extern "C" {
#endif

#define ZIRA_METRICS_MAX_COLS 64
#define ZIRA_METRICS_MAX_HOST 8
#define ZIRA_METRICS_MAX_WINDOW 64
#define ZIRA_METRICS_MAX_RANKS 8
#define ZIRA_METRICS_MAX_ROWS 65536

typedef struct zira_metrics_sources {
    const float *src[ZIRA_METRICS_MAX_COLS]; /* device scalars, the first n_dev are read */
    float host[ZIRA_METRICS_MAX_HOST];       /* host values, the first n_host are stored behind them */
    int32_t n_dev, n_host, n_loss;
} zira_metrics_sources;

int zira_metrics_record_f32(const zira_metrics_sources *sources, float *ring, int rows, int64_t *cursor, int64_t *first_bad,
                            void *stream);

int zira_metrics_window_f64(const float *rings, int64_t rank_stride, int ranks, int rows, int cols, const int64_t *cursor,
                            int window, int n_loss, int max_col, double *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ZIRA_METRICS_H_ */
