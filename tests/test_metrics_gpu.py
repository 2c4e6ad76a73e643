"""The metrics log on the GPU: csrc/metrics.hip against metrics.record_reference / window_reference (numpy), bit for bit --
the oracle is numpy, so there is no tolerance -- the entry points' rejections, graph capture of a record, and the trainer's
``metrics=`` on the small model."""
import ctypes

import numpy as np
import pytest
import torch

from metrics_cases import CASE_IDS, CASES, draw, names_of

from ziragroundingdino_amd import _lib, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_case(case, values):
    """The case's ``values`` [ranks, records, cols] through one native log per rank and through the reference:
    (logs on the device, reference logs)."""
    cols, n_host, n_loss, rows, window, records, ranks = case
    n_dev = cols - n_host
    device_values = torch.from_numpy(values).to(DEV)
    cpu_values = torch.from_numpy(values)
    native, reference = [], []
    for r in range(ranks):
        m = metrics.DeviceMetrics(names_of(case), n_loss, window=window, rows=rows, device=DEV, n_host=n_host)
        assert m.native
        log = metrics.new_reference_log(rows)
        for t in range(records):
            host = [float(h) for h in values[r, t, n_dev:]]
            m.record([device_values[r, t, c] for c in range(n_dev)], host)
            metrics.record_reference(log, [cpu_values[r, t, c] for c in range(n_dev)], host, n_loss)
        native.append(m)
        reference.append(log)
    return native, reference


def reduce(native):
    """The window of rank 0's log over every rank's state buffer (what flush's all_gather assembles)."""
    gathered = torch.stack([m._buf for m in native]).contiguous() if len(native) > 1 else None
    return native[0]._window_native(gathered)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_record_and_window_equal_numpy_bit_for_bit(case):
    cols, n_host, n_loss, rows, window, records, ranks = case
    native, reference = run_case(case, draw(case))
    for m, log in zip(native, reference):
        head = m._head.cpu().tolist()
        assert head == [log["cursor"], log["first_bad"]] == [records, -1]
        ring = m._ring.cpu().numpy()
        for back in range(1, min(rows, records) + 1):          # the ring holds the bits of the latest rows, each in its slot
            want = np.array(log["rows"][-back], dtype=np.float64).astype(np.float32)
            assert np.array_equal(ring[(records - back) % rows].view(np.int32), want.view(np.int32)), back
    out, cursor, first_bad = reduce(native)
    want = metrics.window_reference(reference, window, n_loss, native[0].max_col)
    assert cursor == records and first_bad == -1
    assert out.shape == want.shape == (3, cols + 1) and not np.isnan(want).any()
    for i, kind in enumerate(("latest", "median", "mean")):
        assert np.array_equal(bits64(out[i]), bits64(want[i])), (kind, out[i], want[i])
    if ranks == 1:
        got = native[0].flush(iteration=1000 + records)
        assert got["iteration"] == 1000 + records and got["cursor"] == records
        assert [got["median"][k] for k in names_of(case) + ["total_loss"]] == want[1].tolist()


def test_non_finite_values():
    """A NaN, a +inf and a +inf / -inf pair in different loss columns and an inf in a non-loss column: first_bad is the first
    row with a bad LOSS and sticks; the window's NaNs stand where numpy's stand (their payload is not promised) and every
    other element is numpy's bit for bit."""
    case = (6, 1, 4, 8, 8, 7, 1)
    values = draw(case)
    values[0, 1, 4] = np.inf            # grad_norm-like column: not a loss
    values[0, 3, 2] = np.inf            # the first bad loss
    values[0, 4, 0] = np.nan
    values[0, 5, 1], values[0, 5, 3] = np.inf, -np.inf
    native, reference = run_case(case, values)
    assert native[0]._head.cpu().tolist() == [7, 3] and reference[0]["first_bad"] == 3
    out, cursor, first_bad = reduce(native)
    want = metrics.window_reference(reference, 8, 4, native[0].max_col)
    assert (cursor, first_bad) == (7, 3)
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(want).any() and np.isinf(want).any()
    keep = ~np.isnan(want)
    assert np.array_equal(bits64(out[keep]), bits64(want[keep]))
    with pytest.raises(FloatingPointError, match=r"Loss became infinite or NaN at iteration=503!\nloss_dict = \{'loss_0'"):
        native[0].flush(iteration=506)
    # two ranks, the other one clean until later: the earliest bad iteration of any rank
    clean = draw(case)
    clean[0, 6, 0] = np.nan
    other, other_ref = run_case(case, clean)
    assert other[0]._head.cpu().tolist() == [7, 6]
    out2, _, first_bad2 = reduce([other[0], native[0]])
    assert first_bad2 == 3 == metrics.first_bad_reference([other_ref[0], reference[0]])


def test_before_the_first_record():
    m = metrics.DeviceMetrics(["loss", "lr"], 1, window=4, device=DEV, n_host=1)
    out, cursor, first_bad = m._window_native()
    assert np.isnan(out).all() and out.shape == (3, 3) and (cursor, first_bad) == (0, -1)
    assert m.flush() == {}


def test_rejections_launch_nothing():
    """ZIRA_MSDA_EINVAL for 0 and 65 columns, window 0 and 65, ranks 0 and 9, a null or misaligned pointer; ring, cursor,
    first_bad and out stay as they were."""
    lib, EINVAL = _lib.load(), _lib.CONSTANTS["ZIRA_MSDA_EINVAL"]
    rows = 70
    ring = torch.full((rows * 64,), 7.0, device=DEV)
    head = torch.tensor([5, -1], dtype=torch.int64, device=DEV)
    out = torch.full((3 * 65,), -3.0, dtype=torch.float64, device=DEV)
    src = torch.arange(64, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def sources(n_dev, n_host, n_loss, null_at=None, odd_at=None):
        s = _lib.MetricsSources()
        for i in range(min(n_dev, 64)):
            s.src[i] = src.data_ptr() + 4 * i
        if null_at is not None:
            s.src[null_at] = None
        if odd_at is not None:
            s.src[odd_at] = src.data_ptr() + 2
        s.n_dev, s.n_host, s.n_loss = n_dev, n_host, n_loss
        return ctypes.byref(s)

    cur, bad = head.data_ptr(), head.data_ptr() + 8
    record = lib.zira_metrics_record_f32
    assert record(sources(0, 0, 0), ring.data_ptr(), rows, cur, bad, stream) == EINVAL            # 0 columns
    assert record(sources(65, 0, 0), ring.data_ptr(), rows, cur, bad, stream) == EINVAL           # 65 columns
    assert record(sources(60, 5, 0), ring.data_ptr(), rows, cur, bad, stream) == EINVAL           # 65 columns, 5 from the host
    assert record(sources(3, 9, 0), ring.data_ptr(), rows, cur, bad, stream) == EINVAL            # 9 host values
    assert record(sources(3, 1, 5), ring.data_ptr(), rows, cur, bad, stream) == EINVAL            # more losses than columns
    assert record(sources(3, 0, 3), None, rows, cur, bad, stream) == EINVAL                       # a null ring
    assert record(sources(3, 0, 3), ring.data_ptr(), 0, cur, bad, stream) == EINVAL
    assert record(sources(3, 0, 3), ring.data_ptr(), rows, None, bad, stream) == EINVAL
    assert record(sources(3, 0, 3), ring.data_ptr(), rows, cur, cur + 4, stream) == EINVAL        # misaligned first_bad
    assert record(sources(3, 0, 3, null_at=1), ring.data_ptr(), rows, cur, bad, stream) == EINVAL
    assert record(sources(3, 0, 3, odd_at=2), ring.data_ptr(), rows, cur, bad, stream) == EINVAL
    assert record(None, ring.data_ptr(), rows, cur, bad, stream) == EINVAL
    window = lib.zira_metrics_window_f64
    good = dict(rings=ring.data_ptr(), rank_stride=rows * 64, ranks=1, rows=rows, cols=64, cursor=cur, window=64, n_loss=3,
                max_col=-1, out=out.data_ptr())
    order = ("rings", "rank_stride", "ranks", "rows", "cols", "cursor", "window", "n_loss", "max_col", "out")
    for change in (dict(cols=0), dict(cols=65), dict(window=0), dict(window=65), dict(ranks=0), dict(ranks=9), dict(rings=None),
                   dict(out=None), dict(cursor=None), dict(rows=63), dict(n_loss=65), dict(max_col=2), dict(max_col=64),
                   dict(ranks=2, rank_stride=rows * 64 - 1), dict(out=out.data_ptr() + 4)):
        args = dict(good, **change)
        assert window(*[args[k] for k in order], stream) == EINVAL, change
    torch.cuda.synchronize()
    assert bool((ring == 7.0).all()) and head.cpu().tolist() == [5, -1] and bool((out == -3.0).all())
    assert window(*[good[k] for k in order], stream) == 0                                           # ... and the good call is served
    assert record(sources(64, 0, 3), ring.data_ptr(), rows, cur, bad, stream) == 0
    torch.cuda.synchronize()
    assert head.cpu().tolist() == [6, -1] and ring.view(rows, 64)[5].cpu().tolist() == list(range(64))
    assert bool((ring.view(rows, 64)[:5] == 7.0).all()) and bool((ring.view(rows, 64)[6:] == 7.0).all())
    assert out.view(3, 65)[0, :4].cpu().tolist() == [7.0, 7.0, 7.0, 7.0] and float(out.view(3, 65)[0, 64]) == 21.0


def test_record_is_capturable():
    """One captured record, static sources: three replays with the sources rewritten between them give three distinct rows
    and cursor = 3 (the cursor lives on the device, so nothing of the launch is stale)."""
    m = metrics.DeviceMetrics(["loss_a", "loss_b", "lr"], 2, window=4, device=DEV, n_host=1)
    static = torch.zeros(2, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.record([static[0], static[1]], [0.5])
    assert m._head.cpu().tolist() == [0, -1]                     # captured, not run
    for i in range(3):
        static.copy_(torch.tensor([1.0 + i, 10.0 * (i + 1)]))
        graph.replay()
    torch.cuda.synchronize()
    assert m._head.cpu().tolist() == [3, -1]
    assert m._ring.cpu().tolist() == [[1.0, 10.0, 0.5], [2.0, 20.0, 0.5], [3.0, 30.0, 0.5], [0.0, 0.0, 0.0]]
    got = m.flush()
    assert got["cursor"] == 3 and got["median"]["total_loss"] == 22.0 and got["latest"]["total_loss"] == 33.0


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def _small_trainer(**kw):
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import ZiraTrainer

    return ZiraTrainer(small_model().train(), **kw)


def test_trainer_with_metrics_is_the_trainer_without_and_logs_the_reference_s_numbers():
    from ziragroundingdino_amd.train import synthetic_batch

    data = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, device=DEV)
    logged, plain = _small_trainer(metrics=dict(period=3)), _small_trainer()
    returned = []
    for i in range(3):
        assert logged.last_metrics is None
        a, b = logged.run_step(data), plain.run_step(data)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        returned.append(a)
    for p, q in zip(logged.params, plain.params):
        assert torch.equal(p, q)
    assert logged._metrics_log.native and plain.last_metrics is None and plain._metrics_log is None
    # the reference's bookkeeping over the three returned loss dicts
    log = metrics.new_reference_log(20)
    for d in returned:
        metrics.record_reference(log, list(d.values()))
    want = metrics.window_reference([log], 20, len(returned[0]))
    got = logged.last_metrics
    keys = list(returned[0])
    assert got["iteration"] == 2 and got["cursor"] == 3 and got["loss_names"] == keys
    assert list(got["median"])[len(keys):] == ["grad_norm", "lr", "data_time", "total_loss"]
    for i, kind in enumerate(("latest", "median", "mean")):
        assert np.array_equal(bits64([got[kind][k] for k in keys + ["total_loss"]]), bits64(want[i]))
    assert got["latest"]["grad_norm"] == float(logged.last_grad_norm) and got["latest"]["lr"] == float(np.float32(
        max(logged.optimizer.param_groups, key=lambda g: len(g["params"]))["lr"]))


def test_forced_nan_raises_at_the_flush_naming_the_iteration(monkeypatch):
    """The NaN is written into a recorded source -- the first loss tensor of the second iteration, overwritten in place right
    before it is recorded; the model is not touched.  The error surfaces at the flush (iteration 3), naming iteration 1."""
    from ziragroundingdino_amd.train import synthetic_batch

    data = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, device=DEV)
    trainer = _small_trainer(metrics=dict(period=4))
    original, calls = metrics.DeviceMetrics.record, []

    def record(self, tensors, host_values=()):
        if len(calls) == 1:
            tensors[0].detach().fill_(float("nan"))
        calls.append(1)
        return original(self, tensors, host_values)

    monkeypatch.setattr(metrics.DeviceMetrics, "record", record)
    for _ in range(3):
        trainer.run_step(data)                       # iteration 1 is bad; nothing is read, nothing raised
    with pytest.raises(FloatingPointError, match=r"Loss became infinite or NaN at iteration=1!\nloss_dict = \{") as e:
        trainer.run_step(data)
    assert "nan" in str(e.value) and trainer.last_metrics is None
    assert trainer._metrics_log._head.cpu().tolist() == [4, 1]
