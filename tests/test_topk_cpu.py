"""``topk.topk_rows`` without a GPU: CPU tensors take the sort that defines the op (first k of a stable descending sort: ties by
ascending index, -0.0 == +0.0, NaN first), and the host-side workspace query of csrc/topk.hip answers the served shapes."""
import torch

from ziragroundingdino_amd import _lib, topk


def _definition(x, k):
    """The definition spelled out element by element (no torch.sort)."""
    vals, idxs = [], []
    for row in x.tolist():
        def rank(i):
            v = row[i]
            return (0, 0.0, i) if v != v else (1, -v, i)      # NaN first; then descending (-0.0 == 0.0); then by index
        order = sorted(range(len(row)), key=rank)[:k]
        idxs.append(order)
        vals.append([row[i] for i in order])
    return torch.tensor(vals, dtype=x.dtype).view(x.shape[0], k), torch.tensor(idxs, dtype=torch.int64).view(x.shape[0], k)


def _check(x, k):
    val, idx = topk.topk_rows(x, k)
    want_val, want_idx = _definition(x, k)
    assert idx.dtype == torch.int64 and val.dtype == x.dtype and idx.shape == (x.shape[0], k)
    assert torch.equal(idx, want_idx)
    assert torch.equal(val.view(torch.int32), want_val.view(torch.int32))      # bit patterns: the signs of zeros, NaNs
    assert torch.equal(val.view(torch.int32), torch.gather(x, 1, idx).view(torch.int32))


def test_cpu_tensors_follow_the_stable_sort_definition():
    g = torch.Generator().manual_seed(0)
    assert not topk.supported(torch.zeros(2, 8), 3)
    _check(torch.randn(3, 200, generator=g), 17)
    _check(torch.randn(2, 50, generator=g), 50)                                 # n = k
    x = torch.full((1, 64), -100.0)                                             # all equal: indices 0 .. k-1
    _check(x, 9)
    assert topk.topk_rows(x, 9)[1].tolist() == [list(range(9))]
    x = torch.tensor([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0]])            # the zeros tie whatever their sign
    _check(x, 6)
    assert topk.topk_rows(x, 6)[1].tolist() == [[2, 0, 1, 3, 4, 6]]
    x = torch.randn(2, 40, generator=g)
    x[0, 7] = x[0, 31] = x[1, 0] = float("nan")
    x[0, 3] = float("inf")
    _check(x, 5)
    assert topk.topk_rows(x, 5)[1][0, :3].tolist() == [7, 31, 3]
    _check(torch.randint(0, 4, (4, 300), generator=g).float(), 123)             # heavy ties


def test_other_dtypes_take_the_same_definition():
    x = torch.tensor([[3, 1, 3, 2, 3, 0]], dtype=torch.float64)
    val, idx = topk.topk_rows(x, 4)
    assert idx.tolist() == [[0, 2, 4, 3]] and val.dtype == torch.float64


def test_workspace_query_answers_without_a_gpu():
    lib = _lib.load()
    for shape in ((2, 22223, 900), (2, 900 * 7, 300), (2, 900 * 256, 300), (1, 1024, 1024), (65535, 1 << 20, 1)):
        assert lib.zira_topk_rows_workspace_bytes(*shape) > 0, shape
    for shape in ((2, 22223, 1025), (2, (1 << 20) + 1, 300), (2, 100, 101), (2, 100, 0), (0, 100, 10), (65536, 100, 10)):
        assert lib.zira_topk_rows_workspace_bytes(*shape) == 0, shape
    # argument errors are reported before any launch
    assert lib.zira_topk_rows_f32(None, 2, 100, 10, None, None, None, 0, None) == 1
    assert lib.zira_detections_f32(None, None, 2, 10, 10, 10, None, None, None, None, None, None, 0, None) == 1
