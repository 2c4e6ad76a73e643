"""Training metrics without a per-step host round trip: the reference's ``_write_metrics`` / ``EventStorage`` /
``CommonMetricPrinter`` / ``JSONWriter`` chain (train_multidatasets.py:200, :436-459; detectron2's SimpleTrainer and events.py)
as a ring of fp32 rows on the device.

The reference reads every loss with ``.cpu().item()`` in every iteration, averages over ranks with ``np.mean``, sums into
``total_loss``, checks ``np.isfinite`` and appends to per-key histories that the writers read every 20 iterations as
``np.median`` over the last 20 values.  Here ``DeviceMetrics.record`` is ONE launch (csrc/metrics.hip) that copies the step's
scalars -- device tensors by pointer, host values through the kernel's arguments -- into row ``cursor % rows`` and notes the
first iteration whose losses held an inf / NaN; ``flush`` is one launch that reduces the window in fp64 in numpy's summation
order, and ONE ``.cpu()`` read.  The result is bit for bit what ``record_reference`` / ``window_reference`` -- the reference's
bookkeeping in plain Python and numpy, also the path of CPU tensors, of counts outside the kernels' limits and of
``FORCE_REFERENCE`` -- give for the same numbers.

Two differences from the reference, both documented in README.md: host values (``lr``, ``data_time``) are kept as fp32 like
everything else in the ring, and the ``FloatingPointError`` of a non-finite loss surfaces at the next ``flush``, naming the
iteration it happened in, not inside that iteration (``period=1`` restores the reference's timing at the reference's cost).
"""
import ctypes
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_COLS = _lib.METRICS_CONSTANTS["ZIRA_METRICS_MAX_COLS"]
MAX_HOST = _lib.METRICS_CONSTANTS["ZIRA_METRICS_MAX_HOST"]
MAX_WINDOW = _lib.METRICS_CONSTANTS["ZIRA_METRICS_MAX_WINDOW"]
MAX_RANKS = _lib.METRICS_CONSTANTS["ZIRA_METRICS_MAX_RANKS"]
MAX_ROWS = _lib.METRICS_CONSTANTS["ZIRA_METRICS_MAX_ROWS"]
FORCE_REFERENCE = False     # True: DeviceMetrics keeps its log on the host with record_reference wherever it runs (tests, A/B)
_HEAD_BYTES = 16            # the device state is one buffer: int64 cursor, int64 first_bad, then the ring -- one all_gather moves it


def supported(n_cols, n_host, n_loss, window, rows, device, ranks=1) -> bool:
    """The kernels serve a log of this shape on this device (the limits of include/zira_metrics.h)."""
    return (torch.device(device).type == "cuda" and 1 <= n_cols <= MAX_COLS and 0 <= n_host <= min(MAX_HOST, n_cols)
            and 0 <= n_loss <= n_cols - n_host and 1 <= window <= min(MAX_WINDOW, rows) and rows <= MAX_ROWS
            and 1 <= ranks <= MAX_RANKS)


# ---- the reference's bookkeeping ---------------------------------------------------------------------------------------------
def new_reference_log(rows):
    return {"rows": [], "max_rows": int(rows), "cursor": 0, "first_bad": -1}


def record_reference(log, tensors, host_values=(), n_loss=None):
    """``metrics_dict = {k: v.detach().cpu().item()}`` of one iteration, appended to ``log`` (``new_reference_log``): a list of
    Python floats, the tensors' then the host values' (those as the fp32 the ring would hold).  ``n_loss`` leading entries are
    losses (default: every tensor); ``first_bad`` becomes this iteration's index where their sum is not finite -- the
    reference's ``np.isfinite(sum(...))`` on this rank's own numbers -- and is still -1."""
    row = [float(v) for v in tensors] + [float(np.float32(h)) for h in host_values]
    n_loss = len(tensors) if n_loss is None else n_loss
    if log["first_bad"] < 0 and not np.isfinite(sum(row[:n_loss])):
        log["first_bad"] = log["cursor"]
    log["rows"].append(row)
    del log["rows"][:-log["max_rows"]]
    log["cursor"] += 1
    return row


def rank_mean_reference(rank_rows, n_loss, max_col=-1):
    """One iteration's rows of every rank as the reference reduces them: ``np.mean`` over ranks per key, ``np.max`` for
    ``data_time`` (``max_col``), and ``total_loss = sum(metrics_dict.values())`` over the losses, appended last."""
    cols = len(rank_rows[0])
    with np.errstate(invalid="ignore"):      # (inf + -inf is the NaN the check is there to find)
        x = [(np.max if c == max_col else np.mean)([r[c] for r in rank_rows]) for c in range(cols)]
        return x + [sum(x[:n_loss])]


def window_reference(rank_logs, window, n_loss, max_col=-1):
    """``out`` [3, cols + 1] float64 as zira_metrics_window_f64 defines it, from the rows that the logs of every rank hold:
    latest value, ``np.median`` and ``np.mean`` over the last ``min(window, cursor)`` iterations of the rank-reduced values."""
    rows = [log["rows"] for log in rank_logs]
    cols = len(rows[0][0]) if rows[0] else 0
    n = min(window, rank_logs[0]["cursor"], len(rows[0]))
    out = np.full((3, cols + 1), np.nan, dtype=np.float64)
    if n == 0:
        return out
    hist = [rank_mean_reference([r[len(r) - n + i] for r in rows], n_loss, max_col) for i in range(n)]
    for c in range(cols + 1):
        values = [h[c] for h in hist]
        with np.errstate(invalid="ignore"):
            out[0, c], out[1, c], out[2, c] = values[-1], np.median(values), np.mean(values)
    return out


def first_bad_reference(rank_logs):
    """The first iteration whose rank-averaged total is not finite: the earliest ``first_bad`` of any rank, or -1."""
    bad = [log["first_bad"] for log in rank_logs if log["first_bad"] >= 0]
    return min(bad) if bad else -1


# ---- the log -----------------------------------------------------------------------------------------------------------------
class DeviceMetrics:
    """``names``: the columns in order -- first the tensors' (the ``n_loss`` losses leading), then the host values'.
    ``record(tensors, host_values)`` appends one iteration; ``flush()`` returns
    ``{"iteration", "cursor", "loss_names", "latest": {name: float}, "median": {...}, "mean": {...}}`` over the last ``window``
    iterations, ``total_loss`` among the names, or ``{}`` before the first record.  ``max_name``: the column reduced over ranks
    with a maximum instead of a mean (the reference's ``data_time``)."""

    def __init__(self, names: Sequence[str], n_loss: int, window: int = 20, rows: Optional[int] = None, device="cpu",
                 n_host: int = 0, max_name: Optional[str] = "data_time"):
        self.names = list(names)
        assert len(set(self.names)) == len(self.names) and "total_loss" not in self.names and len(self.names) >= 1
        self.n_loss, self.window, self.n_host = int(n_loss), int(window), int(n_host)
        self.rows = int(rows) if rows is not None else self.window
        assert 1 <= self.window <= self.rows and 0 <= self.n_host <= len(self.names)
        assert 0 <= self.n_loss <= len(self.names) - self.n_host
        self.device = torch.device(device)
        self.max_col = self.names.index(max_name) if max_name in self.names else -1
        assert self.max_col == -1 or self.max_col >= self.n_loss, "a loss is averaged over ranks, not maximised"
        cols = len(self.names)
        self.native = not FORCE_REFERENCE and supported(cols, self.n_host, self.n_loss, self.window, self.rows, self.device)
        if self.native:
            _lib.load()
            nbytes = (_HEAD_BYTES + 4 * self.rows * cols + 15) // 16 * 16
            self._buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            self._head = self._buf[:_HEAD_BYTES].view(torch.int64)          # cursor, first_bad
            self._head.copy_(torch.tensor([0, -1], dtype=torch.int64))
            self._ring = self._buf[_HEAD_BYTES:_HEAD_BYTES + 4 * self.rows * cols].view(torch.float32).view(self.rows, cols)
            self._out = torch.empty(3, cols + 1, dtype=torch.float64, device=self.device)
            self._sources = _lib.MetricsSources()
        else:
            self._log = new_reference_log(self.rows)

    # ---- record ------------------------------------------------------------------------------------------------------------
    def record(self, tensors, host_values=()):
        """Append one iteration.  ``tensors``: one-element tensors (or a dict of them, in ``names`` order), ``host_values``:
        Python numbers.  Native: one launch on the current stream, no host synchronisation; capturable where the tensors are
        static."""
        if isinstance(tensors, dict):
            tensors = [tensors[k] for k in self.names[:len(self.names) - self.n_host]]
        tensors, host_values = list(tensors), list(host_values)
        if len(tensors) + len(host_values) != len(self.names) or len(host_values) != self.n_host:
            raise ValueError("record: %d tensors and %d host values for columns %r (%d of them host values)"
                             % (len(tensors), len(host_values), self.names, self.n_host))
        if not self.native:
            record_reference(self._log, [t.detach() if torch.is_tensor(t) else t for t in tensors], host_values, self.n_loss)
            return
        keep = []
        s = self._sources
        for i, t in enumerate(tensors):
            if not (torch.is_tensor(t) and t.numel() == 1 and t.device == self._buf.device):
                raise ValueError("record: column %r is not a one-element tensor on %s" % (self.names[i], self._buf.device))
            t = t.detach()
            if t.dtype != torch.float32:
                t = t.to(torch.float32)
            keep.append(t)
            s.src[i] = t.data_ptr()
        for i, h in enumerate(host_values):
            s.host[i] = float(h)
        s.n_dev, s.n_host, s.n_loss = len(tensors), len(host_values), self.n_loss
        with torch.cuda.device(self._buf.device):
            rc = _lib.load().zira_metrics_record_f32(ctypes.byref(s), self._ring.data_ptr(), self.rows, self._head.data_ptr(),
                                                     self._head.data_ptr() + 8, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_metrics_record_f32 failed: code %d" % rc)

    # ---- flush -------------------------------------------------------------------------------------------------------------
    def _world(self, process_group):
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(process_group)

    def _gather(self, process_group, world):
        """Every rank's state buffer, [world, bytes] (one all_gather), or None for one rank."""
        if world == 1:
            return None
        import torch.distributed as dist

        gathered = torch.empty(world, self._buf.numel(), dtype=torch.uint8, device=self._buf.device)
        dist.all_gather_into_tensor(gathered, self._buf, group=process_group)
        return gathered

    def _window_native(self, gathered=None):
        """(out [3, cols + 1] float64, cursor, first_bad) over this log or over ``gathered`` state buffers [ranks, bytes] written
        under the same cursor: one launch, one read."""
        cols, world = len(self.names), 1
        rings, stride, heads = self._ring.data_ptr(), 0, self._head
        if gathered is not None:
            world = gathered.shape[0]
            assert gathered.is_contiguous() and gathered.shape[1] == self._buf.numel() and gathered.dtype == torch.uint8
            rings, stride = gathered.data_ptr() + _HEAD_BYTES, self._buf.numel() // 4
            heads = gathered[:, :_HEAD_BYTES].contiguous().view(torch.int64).reshape(-1)
        with torch.cuda.device(self._buf.device):
            rc = _lib.load().zira_metrics_window_f64(rings, stride, world, self.rows, cols, self._head.data_ptr(), self.window,
                                                     self.n_loss, self.max_col, self._out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("zira_metrics_window_f64 failed: code %d" % rc)
        host = torch.cat([self._out.view(torch.int64).reshape(-1), heads]).cpu().numpy()      # the one read
        out = host[:3 * (cols + 1)].view(np.float64).reshape(3, cols + 1)
        heads = host[3 * (cols + 1):].reshape(-1, 2)
        bad = [int(b) for b in heads[:, 1] if b >= 0]
        return out, int(heads[0, 0]), (min(bad) if bad else -1)

    def _bad_row_native(self, first_bad, cursor, gathered):
        if cursor - first_bad > self.rows:
            return None      # overwritten since: flush at least every ``rows`` iterations to see it
        r = first_bad % self.rows
        ring = self._ring[r][None] if gathered is None else torch.stack(
            [g[_HEAD_BYTES:_HEAD_BYTES + 4 * self._ring.numel()].view(torch.float32).view_as(self._ring)[r] for g in gathered])
        return [[float(v) for v in row] for row in ring.cpu().numpy().astype(np.float64)]

    def flush(self, process_group=None, iteration: Optional[int] = None) -> Dict:
        """Reduce the window over the ranks of ``process_group`` and read it: one launch and one ``.cpu()`` (with more than one
        rank, one ``all_gather`` before them).  ``iteration``: the number of the latest recorded iteration (default: its index
        in this log).  Raises ``FloatingPointError`` with the reference's message where a loss was not finite."""
        world = self._world(process_group)
        native = self.native and world <= MAX_RANKS
        if native:
            gathered = self._gather(process_group, world)
            out, cursor, first_bad = self._window_native(gathered)
        else:
            logs = [self._host_log()]
            if world > 1:
                import torch.distributed as dist

                logs = [None] * world
                dist.all_gather_object(logs, self._host_log(), group=process_group)
            out, cursor, first_bad = window_reference(logs, self.window, self.n_loss, self.max_col), logs[0]["cursor"], first_bad_reference(logs)
        if cursor == 0:
            return {}
        iteration = cursor - 1 if iteration is None else int(iteration)
        if first_bad >= 0:
            if native:
                rank_rows = self._bad_row_native(first_bad, cursor, gathered)
            else:
                back = cursor - first_bad
                rank_rows = [log["rows"][-back] for log in logs] if back <= len(logs[0]["rows"]) else None
            loss_dict = None
            if rank_rows is not None:
                loss_dict = dict(zip(self.names[:self.n_loss], rank_mean_reference(rank_rows, self.n_loss, self.max_col)))
            raise FloatingPointError("Loss became infinite or NaN at iteration=%d!\nloss_dict = %s"
                                     % (iteration - (cursor - 1 - first_bad), loss_dict))
        keys = self.names + ["total_loss"]
        result = {"iteration": iteration, "cursor": cursor, "loss_names": self.names[:self.n_loss]}
        for i, kind in enumerate(("latest", "median", "mean")):
            result[kind] = {k: float(out[i, c]) for c, k in enumerate(keys)}
        return result

    def _host_log(self):
        """This rank's log as ``record_reference`` keeps it (a native log is read back: ranks beyond the kernel's limit)."""
        if not self.native:
            return self._log
        head = self._head.cpu()
        cursor, n = int(head[0]), min(int(head[0]), self.rows)
        ring = self._ring.cpu().numpy().astype(np.float64)
        rows = [[float(v) for v in ring[t % self.rows]] for t in range(cursor - n, cursor)]
        return {"rows": rows, "max_rows": self.rows, "cursor": cursor, "first_bad": int(head[1])}


# ---- the writers -------------------------------------------------------------------------------------------------------------
class JSONWriter:
    """detectron2's ``metrics.json``: one JSON object per line, ``iteration`` and the smoothed (median over the window) value of
    every scalar, keys sorted; ``lr`` is written as its latest value, as the reference's scheduler hook asks
    (``smoothing_hint=False``).  Consumes ``DeviceMetrics.flush()``'s dict."""

    def __init__(self, path, window: int = 20, unsmoothed=("lr",)):
        self.path, self.window, self.unsmoothed = path, int(window), tuple(unsmoothed)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._file = open(path, "a")

    def line(self, metrics: Dict) -> str:
        scalars = {k: (metrics["latest"][k] if k in self.unsmoothed else v) for k, v in metrics["median"].items()}
        scalars["iteration"] = metrics["iteration"]
        return json.dumps(scalars, sort_keys=True)

    def write(self, metrics: Dict):
        if metrics:
            self._file.write(self.line(metrics) + "\n")
            self._file.flush()

    def close(self):
        self._file.close()


class CommonMetricPrinter:
    """One line per flush: ``iter``, ``total_loss`` and every loss as the window's median, then ``lr`` (latest), ``data_time``
    and ``grad_norm`` (medians) where the log has them.  Consumes ``DeviceMetrics.flush()``'s dict."""

    def __init__(self, max_iter: Optional[int] = None, emit=None):
        self.max_iter = max_iter
        self.emit = emit if emit is not None else print

    def line(self, metrics: Dict) -> str:
        median, latest = metrics["median"], metrics["latest"]
        it = "%d" % metrics["iteration"] if self.max_iter is None else "%d/%d" % (metrics["iteration"], self.max_iter)
        parts = ["iter: " + it, "total_loss: %.4g" % median["total_loss"]]
        parts += ["%s: %.4g" % (k, median[k]) for k in metrics["loss_names"]]
        if "lr" in latest:
            parts.append("lr: %.5g" % latest["lr"])
        if "data_time" in median:
            parts.append("data_time: %.4f" % median["data_time"])
        if "grad_norm" in median:
            parts.append("grad_norm: %.4g" % median["grad_norm"])
        return "  ".join(parts)

    def write(self, metrics: Dict):
        if metrics:
            self.emit(self.line(metrics))

    def close(self):
        pass
