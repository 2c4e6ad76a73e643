"""``zira_phrase_match_f32`` on the GPU (csrc/phrasematch.hip): every output element bit for bit that of ``match_reference`` on
the device and of phrase_oracle (which the CPU tests pin the reference to), nothing masked out; the kernel -- not the reference --
served the calls; rows of ``prob`` that are not 16-byte aligned; every element written; capture and replay; the evaluator's
device state against the evaluator on CPU state, with no synchronising call before ``evaluate()``."""
import ctypes

import numpy as np
import pytest
import torch

import phrase_cases as cases
from test_phrase_cpu import StubModel, _counts, _dataset

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import phrase_evaluation as pe  # noqa: E402

DEV = "cuda"


@pytest.fixture
def launches(monkeypatch):
    """Counts the calls that reach the kernel's launcher."""
    calls = []
    real = pe._launch
    monkeypatch.setattr(pe, "_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("merged", (False, True))
@pytest.mark.parametrize("name", cases.names())
def test_kernel_equals_the_definition_everywhere(name, merged, launches):
    case = cases.get(name)
    args = cases.tensors(case, DEV) + (case["k_max"], case["iou_thrs"], merged)
    assert pe.match_supported(*args)
    got = cases.as_numpy(pe.match(*args))
    assert len(launches) == 1                                                    # the kernel served the call
    cases.assert_equal(got, cases.as_numpy(pe.match_reference(*args)), (name, merged, "match_reference on the device"))
    assert len(launches) == 1
    cases.assert_equal(got, cases.expected(name, merged), (name, merged, "oracle"))
    again = cases.as_numpy(pe.match(*args))
    cases.assert_equal(again, got, (name, merged, "second run"))


def test_force_reference_and_declined_inputs_take_the_reference(launches, monkeypatch):
    case = cases.get("q65_t33")
    args = cases.tensors(case, DEV)
    tail = (case["k_max"], case["iou_thrs"], False)
    want = cases.expected("q65_t33", False)
    as64 = (args[0].double(),) + args[1:]
    assert not pe.match_supported(*as64, *tail)                                  # another dtype
    cases.assert_equal(cases.as_numpy(pe.match(*as64, *tail)), want, "fp64 prob")
    assert not pe.match_supported(*args, 33, case["iou_thrs"]) and pe.match(*args, 33, case["iou_thrs"]).top_query.shape[2] == 33
    monkeypatch.setattr(pe, "FORCE_REFERENCE", True)
    assert not pe.match_supported(*args, *tail)
    cases.assert_equal(cases.as_numpy(pe.match(*args, *tail)), want, "FORCE_REFERENCE")
    assert launches == []


@pytest.mark.parametrize("name", ("q64_t32", "q900_t256"))
def test_rows_that_are_not_16_byte_aligned(name, launches):
    """T % 4 == 0 but the tensor starts 4 bytes into an allocation: the token-by-token walk, the same bits."""
    case = cases.get(name)
    args = list(cases.tensors(case, DEV))
    flat = torch.empty(args[0].numel() + 1, dtype=torch.float32, device=DEV)
    shifted = flat[1:].view(args[0].shape)
    shifted.copy_(args[0])
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    args[0] = shifted
    got = cases.as_numpy(pe.match(*args, case["k_max"], case["iou_thrs"], False))
    assert len(launches) == 1
    cases.assert_equal(got, cases.expected(name, False), name)


def test_every_output_element_is_written():
    """The C entry on buffers pre-filled with 0xFF: padding, invalid phrases and the rows behind min(k_max, Q) included."""
    lib = _lib.load()
    for name in ("q20_k32", "q63_t31"):
        case = cases.get(name)
        prob, boxes, sizes, bits, gt, count = cases.tensors(case, DEV)
        (B, Q, T), P, G, K, thrs = prob.shape, bits.shape[1], gt.shape[2], case["k_max"], case["iou_thrs"]
        byte = lambda shape, dt: torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size(),), 0xFF,
                                            dtype=torch.uint8, device=DEV).view(dt).view(shape)
        out = pe.PhraseMatch(byte((B, P, K), torch.int32), byte((B, P, K), torch.float32), byte((B, P, K), torch.float64),
                             byte((B, P, len(thrs)), torch.int32), byte((B, P), torch.uint8))
        rc = lib.zira_phrase_match_f32(prob.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), bits.data_ptr(), gt.data_ptr(),
                                       count.data_ptr(), B, Q, T, P, G, K, (ctypes.c_double * len(thrs))(*thrs), len(thrs), 1,
                                       *(t.data_ptr() for t in out), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        cases.assert_equal(cases.as_numpy(out), cases.expected(name, True), name)


def test_the_launch_replays_from_a_captured_graph():
    """The one kernel captured on one stream; the probabilities, the mask words and the counts are rewritten in place."""
    first, second = cases.get("q65_t33"), cases.get("q63_t31")
    static = cases.tensors(first, DEV)
    tail = (first["k_max"], first["iou_thrs"], False)
    pe.match(*static, *tail)                        # (library load and first launch outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pe.match(*static, *tail)
    graph.replay()
    torch.cuda.synchronize()
    cases.assert_equal(cases.as_numpy(out), cases.expected("q65_t33", False), "replay of the captured inputs")
    # other contents in the same buffers: the first 63 queries and 31 tokens of the other case inside this case's shape
    changed = {k: first[k].copy() for k in cases.INPUTS}
    changed["prob"][:, :63, :31] = second["prob"]
    changed["boxes"][:, :63] = second["boxes"]
    changed["gt_count"][:] = np.array([[2, 0, 5], [1, 4, 0]], np.int32)
    changed["phrase_bits"][:, :, 0] = np.array([[5, 1 << 20, 0], [-2 ** 31, 3, 7]], np.int32)
    for dst, k in zip(static, cases.INPUTS):
        dst.copy_(torch.from_numpy(changed[k]))
    graph.replay()
    torch.cuda.synchronize()
    got = cases.as_numpy(out)
    want = cases.oracle.match(*(changed[k] for k in cases.INPUTS), *tail)
    cases.assert_equal(got, want, "replay of rewritten inputs")
    assert want["valid"].tolist() == [[1, 0, 0], [1, 1, 0]] and not np.array_equal(want["top_query"], cases.expected("q65_t33", False)["top_query"])


def test_the_evaluators_state_stays_on_the_device_until_evaluate(launches):
    case, inputs = _dataset("q900_t256")
    thrs = (0.5, 0.75)
    dev_inputs = [dict(x, phrases=x["phrases"].to(DEV)) for x in inputs]

    class OnDevice(StubModel):
        def forward_grounding(self, batch):
            return {k: v.to(DEV) for k, v in super().forward_grounding(batch).items()}

    ev = pe.PhraseGroundingEvaluator(ks=(1, 5, 10), iou_thrs=thrs)
    model = OnDevice(case).eval()
    with torch.no_grad():
        ev.process(dev_inputs[:1], model.forward_grounding(dev_inputs[:1]))
    assert len(launches) == 1 and list(ev._state) == [torch.device("cuda", torch.cuda.current_device())]
    assert all(t.is_cuda and t.dtype == torch.int64 for t in ev._state[next(iter(ev._state))])
    # the second image from tensors that already are on the device: not one synchronising torch call
    args = tuple(t[1:].contiguous() for t in cases.tensors(case, DEV))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.process_padded(*args)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert len(launches) == 2 and all(t.is_cuda for t in ev._state[next(iter(ev._state))])
    result = ev.evaluate()
    hits, n = _counts(case, (1, 5, 10), thrs, False, 10)
    assert ev.hits == hits and ev.num_valid == n == 61
    assert result["grounding"]["R@5/IoU=0.75"] == 100.0 * hits[1][1] / n and len(result["grounding"]) == 6

    # the same dataset on CPU state, and device state merged with CPU state: the host path, the same numbers
    host = pe.PhraseGroundingEvaluator(ks=(1, 5, 10), iou_thrs=thrs)
    assert pe.inference_on_grounding_dataset(StubModel(case), [inputs], host) == result
    half_dev, half_cpu = (pe.PhraseGroundingEvaluator(ks=(1, 5, 10), iou_thrs=thrs) for _ in range(2))
    with torch.no_grad():
        half_dev.process(dev_inputs[:1], model.forward_grounding(dev_inputs[:1]))
        half_cpu.process(inputs[1:], StubModel(case).eval().forward_grounding(inputs[1:]))
    assert len(half_dev.merge(half_cpu)._state) == 2 and half_dev.evaluate() == result
