"""Shared case table of the metrics-log tests (test_metrics_cpu.py, test_metrics_gpu.py): the shapes at which the record and
window kernels can go wrong, and the values they are fed.

Every case is ``(cols, n_host, n_loss, rows, window, records, ranks)``:
  * cols 1, 31, 33, 64: one lane, below / above half a wave, the whole wave;
  * rows 4 with 9 records: the ring wraps twice and a bit; rows == window elsewhere, and one ring longer than its window;
  * window 1, 2, 19, 20, 64 against fewer, exactly as many and more records: odd / even medians, the pairwise sum's
    sequential (< 8), whole-groups-of-8 (64) and leftover (19, 20) paths;
  * ranks 1, 2, 3 (sequential mean), 8 (numpy's unrolled pairwise path)."""
import numpy as np

CASES = [
    # cols n_host n_loss rows window records ranks
    (1, 0, 1, 4, 1, 9, 1),
    (1, 0, 1, 4, 4, 9, 2),
    (31, 2, 22, 2, 2, 1, 1),
    (31, 2, 22, 2, 2, 2, 3),
    (33, 2, 30, 19, 19, 18, 1),
    (33, 2, 30, 19, 19, 19, 2),
    (33, 8, 25, 19, 19, 23, 1),
    (27, 2, 22, 20, 20, 7, 8),
    (27, 2, 22, 20, 20, 20, 1),
    (27, 2, 22, 20, 20, 41, 3),
    (27, 2, 22, 32, 20, 45, 1),
    (64, 0, 64, 64, 64, 63, 1),
    (64, 2, 40, 64, 64, 64, 1),
    (64, 2, 0, 64, 64, 70, 2),
    (5, 2, 3, 8, 8, 8, 8),
    (5, 2, 3, 9, 9, 13, 8),
]
CASE_IDS = ["c%d_h%d_l%d_r%d_w%d_n%d_k%d" % c for c in CASES]


def draw(case, seed=0):
    """``values`` [ranks, records, cols] float32.  Drawn from a handful of quarters, so that the window's medians fall on ties
    and on the average of two different middle values; host columns (the last n_host) are the same on every rank except the
    last one (data_time, maximised over ranks); one denormal and one negative zero sit in rank 0's latest rows."""
    cols, n_host, n_loss, rows, window, records, ranks = case
    rng = np.random.default_rng(seed + 1000 * cols + records)
    values = rng.integers(0, 7, (ranks, records, cols)).astype(np.float32) * np.float32(0.25)
    values += (rng.integers(0, 4, (ranks, records, cols)) == 0) * rng.standard_normal((ranks, records, cols)).astype(np.float32)
    if n_host > 1:
        values[:, :, cols - n_host:cols - 1] = values[:1, :, cols - n_host:cols - 1]
    values[0, records - 1, 0] = np.float32(1e-41)          # a denormal
    if records > 1:
        values[0, records - 2, cols // 2] = np.float32(-0.0)
    return values.astype(np.float32)


def names_of(case):
    cols, n_host = case[0], case[1]
    names = ["loss_%d" % i for i in range(cols - n_host)] + ["host_%d" % i for i in range(n_host)]
    if n_host:
        names[-1] = "data_time"
    return names
