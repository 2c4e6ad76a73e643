"""The metrics log without a GPU: the reference bookkeeping (metrics.record_reference / window_reference, which is also the
kernels' oracle) against histories worked out by hand, the writers' lines, the second public header and the trainer's
``metrics=`` on CPU tensors, alone and over two gloo ranks."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import ROOT
from metrics_cases import CASE_IDS, CASES, draw

from ziragroundingdino_amd import _header, _lib, metrics
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd.train import ZiraTrainer


def log_of(values, n_loss, window, rows=None, names=None, n_host=0):
    """A CPU DeviceMetrics fed ``values`` [records][cols]."""
    cols = len(values[0])
    m = metrics.DeviceMetrics(names or ["loss_%d" % i for i in range(cols)], n_loss, window=window, rows=rows, n_host=n_host)
    assert not m.native
    for row in values:
        m.record([torch.tensor(v, dtype=torch.float32) for v in row[:cols - n_host]], row[cols - n_host:])
    return m


@pytest.mark.parametrize("window, records, latest, median, mean", [
    (1, 3, 2.0, 2.0, 2.0),                  # values 3, 1, 2
    (2, 3, 2.0, 1.5, 1.5),                  # 1, 2
    (20, 3, 2.0, 2.0, 2.0),                 # a window longer than the history: all of it
    (19, 25, 25.0, 16.0, 16.0),             # values 1 .. 25: the last 19 are 7 .. 25
    (20, 25, 25.0, 15.5, 15.5),             # 6 .. 25
    (20, 20, 20.0, 10.5, 10.5),
])
def test_window_counts_by_hand(window, records, latest, median, mean):
    values = [[3.0], [1.0], [2.0]] if records == 3 else [[float(i + 1)] for i in range(records)]
    got = log_of(values, 1, window).flush()
    assert got["iteration"] == records - 1 and got["cursor"] == records and got["loss_names"] == ["loss_0"]
    for key in ("loss_0", "total_loss"):
        assert (got["latest"][key], got["median"][key], got["mean"][key]) == (latest, median, mean)


def test_ring_wraps():
    """rows = 4, 9 records of (i, 10 i): the ring holds iterations 5 .. 8; the total is their sum per iteration."""
    got = log_of([[float(i), 10.0 * i] for i in range(9)], 2, window=4, rows=4).flush(iteration=108)
    assert got["iteration"] == 108 and got["cursor"] == 9
    assert got["latest"] == {"loss_0": 8.0, "loss_1": 80.0, "total_loss": 88.0}
    assert got["median"] == {"loss_0": 6.5, "loss_1": 65.0, "total_loss": 71.5}
    assert got["mean"] == got["median"]


def test_before_the_first_record_there_is_nothing():
    assert metrics.DeviceMetrics(["loss"], 1).flush() == {}


def test_only_the_leading_columns_are_losses():
    """grad_norm = inf and found_inf = 1 beside finite losses raise nothing; the total is the losses' alone."""
    m = log_of([[1.0, 2.0, math.inf, 1.0], [3.0, 4.0, math.nan, 0.0]], 2, 20, names=["a", "b", "grad_norm", "found_inf"])
    got = m.flush()
    assert got["latest"]["total_loss"] == 7.0 and got["median"]["total_loss"] == 5.0
    assert math.isnan(got["median"]["grad_norm"]) and math.isnan(got["latest"]["grad_norm"])


@pytest.mark.parametrize("bad_row, column", [([math.nan, 1.0, 1.0], "a"), ([1.0, math.inf, 1.0], "b"),
                                             ([math.inf, 1.0, -math.inf], "a")])
def test_non_finite_losses_raise_at_the_flush_and_stick(bad_row, column):
    """A NaN, a +inf, and a +inf / -inf pair (whose sum is a NaN): FloatingPointError with the reference's message, naming
    the iteration of the FIRST bad row; it is raised again by every later flush."""
    rows = [[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], bad_row, [1.0, 1.0, 1.0], [math.nan, math.nan, math.nan]]
    m = log_of(rows, 3, 20, names=["a", "b", "c"])
    for later in range(2):
        with pytest.raises(FloatingPointError) as e:
            m.flush(iteration=104 + later)
        text = str(e.value)
        assert text.startswith("Loss became infinite or NaN at iteration=102!\nloss_dict = {")
        want = bad_row[["a", "b", "c"].index(column)]
        assert "'%s': %s" % (column, "nan" if math.isnan(want) else "inf") in text.replace("np.float64(", "").replace(")", "")
        m.record([torch.tensor(1.0)] * 3)
    assert m._log["first_bad"] == 2


def test_rank_mean_total_and_data_time_maximum():
    """Two ranks by hand: np.mean per key, np.max of data_time, total = the sum of the means."""
    logs = []
    for rank_rows in ([[1.0, 10.0, 0.5], [3.0, 30.0, 0.1]], [[2.0, 20.0, 0.25], [5.0, 50.0, 0.75]]):
        log = metrics.new_reference_log(20)
        for r in rank_rows:
            metrics.record_reference(log, [torch.tensor(v) for v in r[:2]], r[2:], n_loss=2)
        logs.append(log)
    out = metrics.window_reference(logs, 20, 2, max_col=2)
    assert out[0].tolist() == [4.0, 40.0, 0.75, 44.0]
    assert out[1].tolist() == [2.75, 27.5, 0.625, 30.25] and out[2].tolist() == out[1].tolist()
    assert metrics.first_bad_reference(logs) == -1
    logs[1]["first_bad"] = 1
    assert metrics.first_bad_reference(logs) == 1


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reference_is_numpy_over_the_retained_rows(case):
    """window_reference on the shared cases against the same statement written a second way (array reductions over the
    last rows instead of per-iteration lists)."""
    cols, n_host, n_loss, rows, window, records, ranks = case
    values = draw(case)
    logs = []
    for r in range(ranks):
        log = metrics.new_reference_log(rows)
        for t in range(records):
            metrics.record_reference(log, list(torch.from_numpy(values[r, t, :cols - n_host])), values[r, t, cols - n_host:], n_loss)
        logs.append(log)
    max_col = cols - 1 if n_host else -1
    out = metrics.window_reference(logs, window, n_loss, max_col)
    n = min(window, records)
    tail = values[:, records - n:].astype(np.float64)                      # [ranks, n, cols]
    x = np.stack([np.array([np.mean(list(tail[:, i, c])) for c in range(cols)]) for i in range(n)])
    if n_host:
        x[:, max_col] = tail[:, :, max_col].max(0)
    total = np.array([sum(x[i, :n_loss]) for i in range(n)])
    x = np.concatenate([x, total[:, None]], 1)
    assert np.array_equal(out[0].view(np.int64), x[-1].view(np.int64))
    assert np.array_equal(out[1], np.median(x, axis=0))
    assert np.allclose(out[2], x.mean(0), rtol=1e-14, atol=0)
    assert logs[0]["cursor"] == records and len(logs[0]["rows"]) == min(rows, records) and logs[0]["first_bad"] == -1


# ---- the writers -------------------------------------------------------------------------------------------------------------
FLUSHED = {"iteration": 39, "cursor": 40, "loss_names": ["loss_class", "loss_bbox"],
           "latest": {"loss_class": 1.0, "loss_bbox": 0.5, "grad_norm": 3.0, "lr": 0.0001, "data_time": 0.002, "total_loss": 1.5},
           "median": {"loss_class": 1.25, "loss_bbox": 0.625, "grad_norm": 2.0, "lr": 0.001, "data_time": 0.00125, "total_loss": 1.875},
           "mean": {"loss_class": 1.3, "loss_bbox": 0.7, "grad_norm": 2.5, "lr": 0.0007, "data_time": 0.0015, "total_loss": 2.0}}


def test_json_writer_line(tmp_path):
    path = tmp_path / "out" / "metrics.json"
    w = metrics.JSONWriter(str(path))
    w.write(FLUSHED)
    w.write({})                  # nothing recorded yet: nothing written
    w.write(dict(FLUSHED, iteration=59))
    w.close()
    lines = path.read_text().splitlines()
    assert lines[0] == ('{"data_time": 0.00125, "grad_norm": 2.0, "iteration": 39, "loss_bbox": 0.625, "loss_class": 1.25, '
                        '"lr": 0.0001, "total_loss": 1.875}')
    assert len(lines) == 2 and json.loads(lines[1])["iteration"] == 59


def test_printer_line():
    lines = []
    p = metrics.CommonMetricPrinter(90000, emit=lines.append)
    p.write(FLUSHED)
    p.write({})
    assert lines == ["iter: 39/90000  total_loss: 1.875  loss_class: 1.25  loss_bbox: 0.625  lr: 0.0001  data_time: 0.0013  "
                     "grad_norm: 2"]
    assert metrics.CommonMetricPrinter().line(FLUSHED).startswith("iter: 39  total_loss")


# ---- the header --------------------------------------------------------------------------------------------------------------
def test_metrics_header_parses_into_tables_of_its_own():
    with open(os.path.join(ROOT, "include", "zira_metrics.h")) as f:
        protos, structs, consts = _header.parse(f.read(), name="zira_metrics.h")
    assert list(protos) == ["zira_metrics_record_f32", "zira_metrics_window_f64"] == list(_lib.METRICS_SYMBOLS)
    assert consts == _lib.METRICS_CONSTANTS == {"ZIRA_METRICS_MAX_COLS": 64, "ZIRA_METRICS_MAX_HOST": 8, "ZIRA_METRICS_MAX_WINDOW": 64,
                                                "ZIRA_METRICS_MAX_RANKS": 8, "ZIRA_METRICS_MAX_ROWS": 65536}
    vp, i = ctypes.c_void_p, ctypes.c_int
    P = _lib.METRICS_PROTOTYPES
    assert P["zira_metrics_record_f32"] == (i, [ctypes.POINTER(_lib.MetricsSources), vp, i, vp, vp, vp])
    assert P["zira_metrics_window_f64"] == (i, [vp, ctypes.c_int64, i, i, i, vp, i, i, i, vp, vp])
    # sizeof / offsetof as a host C compiler lays the struct out (x86-64): 64 pointers, 8 floats, 3 ints, padded to 8
    S = _lib.MetricsSources
    assert list(_lib.METRICS_STRUCTS) == ["zira_metrics_sources"] and ctypes.sizeof(S) == 560
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == [
        ("src", 0, 512), ("host", 512, 32), ("n_dev", 544, 4), ("n_host", 548, 4), ("n_loss", 552, 4)]


def test_library_exports_the_metrics_symbols_and_types_them():
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.METRICS_PROTOTYPES.items():
        assert hasattr(raw, name), "libzira_msda.so does not export %s" % name
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes
    # argument errors are answered on the host, nothing launched: no GPU needed
    assert lib.zira_metrics_record_f32(None, None, 4, None, None, None) == _lib.CONSTANTS["ZIRA_MSDA_EINVAL"]
    assert lib.zira_metrics_window_f64(None, 0, 1, 4, 4, None, 4, 1, -1, None, None) == 1


def test_the_first_header_s_tables_are_untouched():
    assert len(_lib.SYMBOLS) == 100 and not any("metrics" in s for s in _lib.SYMBOLS)
    assert not any("METRICS" in c for c in _lib.CONSTANTS) and "zira_metrics_sources" not in _lib.STRUCTS
    assert tuple(_lib.PROTOTYPES) == _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "zira_msda.h")) as f:
        assert "metrics" not in f.read().lower()


@pytest.mark.parametrize("text, named", [
    ("typedef struct zira_s { int a[0]; } zira_s;\n", r"bad\.h line 1.*int a\[0\]"),
    ("typedef struct zira_s { int a[ZIRA_NOPE]; } zira_s;\n", r"line 1.*ZIRA_NOPE"),
    ("typedef struct zira_s { int a, b[2]; } zira_s;\n", r"line 1.*int a, b\[2\]"),
    ("int zira_f(int a[2]);\n", r"line 1.*int a\[2\]"),
])
def test_the_reader_takes_member_arrays_only(text, named):
    with pytest.raises(_header.HeaderError, match=named):
        _header.parse(text, name="bad.h")
    _, structs, _ = _header.parse("#define ZIRA_N 3\ntypedef struct zira_s { const float *p[ZIRA_N]; float h[2]; int n; } zira_s;\n")
    assert [(n, ctypes.sizeof(t)) for n, t in structs["zira_s"]._fields_] == [("p", 24), ("h", 8), ("n", 4)]


def test_supported_declines_what_the_kernels_do_not_serve():
    ok = dict(n_cols=27, n_host=2, n_loss=22, window=20, rows=20, device="cuda")
    assert metrics.supported(**ok) and metrics.supported(**dict(ok, ranks=8))
    for change in (dict(device="cpu"), dict(n_cols=65), dict(n_cols=0), dict(n_host=9), dict(n_loss=26), dict(window=0),
                   dict(window=65, rows=65), dict(window=21), dict(rows=65537), dict(ranks=9), dict(ranks=0)):
        assert not metrics.supported(**dict(ok, **change)), change


# ---- the trainer -------------------------------------------------------------------------------------------------------------
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.adapter = nn.Linear(4, 4)

    def before_train(self):
        pass

    def forward(self, x):
        y = self.adapter(x)
        return {"loss_sq": (y * y).mean(), "loss_abs": y.abs().mean()}


def _expected(loss_dicts, window):
    """The reference's bookkeeping over the returned loss dicts of one rank: median / latest / total per key."""
    tail = loss_dicts[-window:]
    rows = [{k: float(v) for k, v in d.items()} for d in tail]
    total = [sum(r.values()) for r in rows]
    return ({k: np.median([r[k] for r in rows]) for k in rows[0]}, rows[-1], np.median(total), total[-1])


def test_cpu_trainer_takes_the_reference_path(tmp_path):
    lines = []
    writers = [metrics.CommonMetricPrinter(6, emit=lines.append), metrics.JSONWriter(str(tmp_path / "metrics.json"))]
    trainer = ZiraTrainer(_Tiny(), tuned_gemms=False, metrics=dict(period=3, window=2, writers=writers))
    plain = ZiraTrainer(_Tiny(), tuned_gemms=False)
    assert plain.metrics is None and plain.last_metrics is None and plain._metrics_log is None
    torch.manual_seed(1)
    batches = [torch.randn(5, 4) for _ in range(6)]
    returned = []
    for i, x in enumerate(batches):
        trainer.data_time = 0.25 * i
        returned.append(trainer.run_step(x))
        for k, v in plain.run_step(x).items():
            assert torch.equal(v, returned[-1][k])                       # the log changes nothing it watches
        if i < 2:
            assert trainer.last_metrics is None
        if i in (2, 5):
            got = trainer.last_metrics
            median, latest, total_median, total_latest = _expected(returned, 2)
            assert got["iteration"] == i and got["loss_names"] == ["loss_sq", "loss_abs"]
            assert list(got["median"]) == ["loss_sq", "loss_abs", "grad_norm", "lr", "data_time", "total_loss"]
            for k in median:
                assert got["median"][k] == median[k] and got["latest"][k] == latest[k]
            assert got["median"]["total_loss"] == total_median and got["latest"]["total_loss"] == total_latest
            assert got["latest"]["data_time"] == 0.25 * i and got["median"]["data_time"] == 0.25 * i - 0.125
            assert got["latest"]["lr"] == float(np.float32(1e-3))
            assert got["latest"]["grad_norm"] == float(trainer.last_grad_norm)
    assert not trainer._metrics_log.native and plain.last_metrics is None
    assert len(lines) == 2 and lines[1].startswith("iter: 5/6  total_loss: ")
    written = [json.loads(s) for s in (tmp_path / "metrics.json").read_text().splitlines()]
    assert [w["iteration"] for w in written] == [2, 5] and written[1]["loss_sq"] == trainer.last_metrics["median"]["loss_sq"]
    for p, q in zip(trainer.params, plain.params):
        assert torch.equal(p, q)


def _rank_worker(rank, world, store, out):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    torch.set_num_threads(1)
    trainer = ZiraTrainer(_Tiny(), tuned_gemms=False, metrics=dict(period=2, window=2))
    torch.manual_seed(10 + rank)
    returned = []
    for i in range(2):
        trainer.data_time = 1.0 + rank + i
        returned.append({k: float(v) for k, v in trainer.run_step(torch.randn(5, 4)).items()})
    torch.save({"returned": returned, "metrics": trainer.last_metrics}, out % rank)
    dist.destroy_process_group()


def test_two_gloo_ranks_give_the_rank_mean_and_the_data_time_maximum(tmp_path):
    import torch.multiprocessing as mp

    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_rank_worker, args=(2, str(tmp_path / "store"), out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0, weights_only=False), torch.load(out % 1, weights_only=False)
    assert r0["metrics"] == r1["metrics"]                  # every rank reduces the same gathered rows
    got = r0["metrics"]
    per_iter = [{k: np.mean([r0["returned"][i][k], r1["returned"][i][k]]) for k in r0["returned"][i]} for i in range(2)]
    totals = [sum(d.values()) for d in per_iter]
    for k in per_iter[0]:
        assert got["latest"][k] == per_iter[1][k] and got["median"][k] == np.median([per_iter[0][k], per_iter[1][k]])
    assert got["latest"]["total_loss"] == totals[1] and got["median"]["total_loss"] == np.median(totals)
    assert got["latest"]["data_time"] == 3.0 and got["median"]["data_time"] == 2.5      # max(1, 2) = 2, max(2, 3) = 3
    assert r0["returned"] != r1["returned"]


def test_task_spec_log_period_writes_metrics_json(tmp_path, capsys):
    from ziragroundingdino_amd.tasks import TaskSpec, run_task

    class _Task(_Tiny):
        def add_cls_prompt(self, names):
            pass

        def after_train(self):
            pass

    data = lambda start: iter([torch.randn(5, 4) for _ in range(4)])      # noqa: E731
    run_task(TaskSpec("logged", ["a"], data, max_iter=4, output_dir=str(tmp_path / "logged"), log_period=2), _Task, None)
    lines = [json.loads(s) for s in (tmp_path / "logged" / "metrics.json").read_text().splitlines()]
    assert [w["iteration"] for w in lines] == [1, 3]
    assert sorted(lines[0]) == ["data_time", "grad_norm", "iteration", "loss_abs", "loss_sq", "lr", "total_loss"]
    assert lines[1]["lr"] == float(np.float32(1e-4))           # the multiplier's x0.1 from iteration 1 on (40 % of 4)
    printed = capsys.readouterr().out.splitlines()
    assert [p.split("  ")[0] for p in printed if p.startswith("iter: ")] == ["iter: 1/4", "iter: 3/4"]
    run_task(TaskSpec("silent", ["a"], data, max_iter=4, output_dir=str(tmp_path / "silent")), _Task, None)
    assert not (tmp_path / "silent" / "metrics.json").exists()
