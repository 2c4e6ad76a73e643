"""The grounding tail on the GPU: ``zira_ground_f32`` (csrc/grounding.hip) through ``grounding.ground`` byte for byte against
the op-chain twin ``ground_reference`` on the same probabilities copied to the CPU -- no tolerance, the contract is bit
identity -- over the shapes and values of tests/grounding_cases.py and both orders; pre-filled outputs, hipGraph replay, the
C entry's refusals, and ``predict`` end to end on the small model with the kernel against the twin."""
import pytest
import torch

import grounding_cases as gc
from test_grounding_cpu import assert_bytes_equal

from ziragroundingdino_amd import _lib, grounding
from ziragroundingdino_amd import transformer as zt

pytestmark = pytest.mark.gpu

EINVAL = 1      # hipErrorInvalidValue


def _cpu(g):
    return grounding.Grounded(*[t.cpu() for t in g])


@pytest.mark.parametrize("case", gc.all_cases(), ids=gc.case_id)
def test_kernel_equals_the_twin_byte_for_byte(case):
    prob, boxes, box_thr, text_thr = gc.make(*case)
    prob_d, boxes_d = prob.cuda(), boxes.cuda()
    assert grounding.supported(prob_d, boxes_d)
    for order in (0, 1):
        got = _cpu(grounding.ground(prob_d, boxes_d, box_thr, text_thr, order))
        want = grounding.ground_reference(prob_d.cpu(), boxes_d.cpu(), box_thr, text_thr, order)
        assert_bytes_equal(got, want, "order %d" % order)
        again = _cpu(grounding.ground(prob_d, boxes_d, box_thr, text_thr, order))
        assert_bytes_equal(again, got, "second run, order %d" % order)


def test_unaligned_rows_take_the_scalar_path():
    """T = 256 rows that do not start on 16 bytes (a view one float into a buffer) are read without the float4 loads."""
    prob, boxes, box_thr, text_thr = gc.make("sparse", 3, 65, 256)
    buf = torch.zeros(prob.numel() + 1, device="cuda")
    view = buf[1:].view(prob.shape)
    view.copy_(prob)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    for order in (0, 1):
        got = _cpu(grounding.ground(view, boxes.cuda(), box_thr, text_thr, order))
        assert_bytes_equal(got, grounding.ground_reference(prob, boxes, box_thr, text_thr, order), "order %d" % order)


def _raw_call(lib, prob, boxes, box_thr, text_thr, order, out, ws):
    B, Q, T = prob.shape
    return lib.zira_ground_f32(prob.data_ptr(), boxes.data_ptr(), B, Q, T, box_thr, text_thr, order, out.query.data_ptr(),
                               out.score.data_ptr(), out.box.data_ptr(), out.argmax_token.data_ptr(),
                               out.token_bits.data_ptr(), out.n_keep.data_ptr(), ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream().cuda_stream)


def _filled(B, Q, T, byte):
    W = (T + 31) // 32

    def make(shape, dtype):
        n = 4
        for d in shape:
            n *= d
        return torch.full((n,), byte, dtype=torch.uint8, device="cuda").view(dtype).view(shape)

    return grounding.Grounded(make((B, Q), torch.int32), make((B, Q), torch.float32), make((B, Q, 4), torch.float32),
                              make((B, Q), torch.int32), make((B, Q, W), torch.int32), make((B,), torch.int32))


@pytest.mark.parametrize("kind,B,Q,T", [("sparse", 3, 65, 33), ("none", 1, 900, 256), ("sparse", 1, 900, 256), ("all", 3, 64, 32)])
def test_prefilled_outputs_come_back_fully_written(kind, B, Q, T):
    prob, boxes, box_thr, text_thr = gc.make(kind, B, Q, T)
    lib = _lib.load()
    ws = torch.empty(lib.zira_ground_workspace_bytes(B, Q, T), dtype=torch.uint8, device="cuda")
    for order in (0, 1):
        out = _filled(B, Q, T, 0xFF)
        assert all(bool((t.view(torch.uint8) == 0xFF).all()) for t in out)
        assert _raw_call(lib, prob.cuda(), boxes.cuda(), box_thr, text_thr, order, out, ws) == 0
        assert_bytes_equal(_cpu(out), grounding.ground_reference(prob, boxes, box_thr, text_thr, order), "order %d" % order)


@pytest.mark.parametrize("order", [0, 1])
def test_capture_and_replay_on_three_inputs(order):
    B, Q, T = 2, 900, 256
    inputs = [gc.make(kind, B, Q, T) for kind in ("sparse", "ties8", "nan")]
    box_thr, text_thr = 0.45, 0.3
    prob_s, boxes_s = torch.zeros(B, Q, T, device="cuda"), torch.zeros(B, Q, 4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up off the default stream, as torch's capture asks
        grounding.ground(prob_s, boxes_s, box_thr, text_thr, order)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = grounding.ground(prob_s, boxes_s, box_thr, text_thr, order)
    for prob, boxes, _, _ in inputs:
        prob_s.copy_(prob)
        boxes_s.copy_(boxes)
        graph.replay()
        torch.cuda.synchronize()
        assert_bytes_equal(_cpu(out), grounding.ground_reference(prob, boxes, box_thr, text_thr, order), "replay")
        assert 0 < int(out.n_keep.min()) and int(out.n_keep.max()) < Q


def test_c_entry_refuses_unsupported_shapes_without_launching():
    lib = _lib.load()
    prob, boxes = torch.rand(2, 8, 16, device="cuda"), torch.rand(2, 8, 4, device="cuda")
    out = _filled(2, 8, 16, 0xFF)
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")

    def call(B, Q, T, order=0, ws_bytes=256, boxes_ptr=None):
        return lib.zira_ground_f32(prob.data_ptr(), boxes_ptr or boxes.data_ptr(), B, Q, T, 0.3, 0.2, order,
                                   out.query.data_ptr(), out.score.data_ptr(), out.box.data_ptr(), out.argmax_token.data_ptr(),
                                   out.token_bits.data_ptr(), out.n_keep.data_ptr(), ws.data_ptr(), ws_bytes,
                                   torch.cuda.current_stream().cuda_stream)

    for B, Q, T in [(0, 8, 16), (65536, 8, 16), (2, 0, 16), (2, 1025, 16), (2, 8, 0), (2, 8, 257)]:
        assert lib.zira_ground_workspace_bytes(B, Q, T) == 0
        assert call(B, Q, T) == EINVAL
    assert call(2, 8, 16, order=2) == EINVAL
    assert call(2, 8, 16, ws_bytes=0) == EINVAL
    assert call(2, 8, 16, boxes_ptr=boxes.data_ptr() + 4) == EINVAL      # a box row moves as 16 bytes
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0xFF).all()) for t in out)   # nothing was launched
    assert call(2, 8, 16) == 0
    torch.cuda.synchronize()
    assert_bytes_equal(_cpu(out), grounding.ground_reference(prob.cpu(), boxes.cpu(), 0.3, 0.2), "after the refusals")
    with pytest.raises(ValueError):
        grounding.ground(prob, boxes, 0.3, 0.2, order=3)
    big = torch.rand(1, 1025, 8, device="cuda")                         # declined shapes take the twin, on the device
    assert not grounding.supported(big, torch.rand(1, 1025, 4, device="cuda"))


def test_predict_end_to_end_kernel_equals_twin(monkeypatch):
    from test_model_gpu import small_model

    from ziragroundingdino_amd.train import synthetic_batch

    model = small_model().eval()
    a = synthetic_batch(1, 224, 320, n_categories=4, boxes_per_image=3, seed=1, device="cuda")[0]
    b = synthetic_batch(1, 200, 272, n_categories=2, boxes_per_image=1, seed=2, device="cuda")[0]
    a["captions"], b["captions"] = "Fish . Jellyfish . Penguin . Puffin", "a shark . starfish ."
    batch = [a, b]
    # the model runs once; the two paths below get the very same logits and boxes (the comparison is of the tails)
    memo, real_forward = {}, model.forward_grounding

    def forward_once(inputs):
        key = tuple(x["captions"] for x in inputs)
        if key not in memo:
            memo[key] = real_forward(inputs)
        return memo[key]

    monkeypatch.setattr(model, "forward_grounding", forward_once)
    with torch.no_grad():
        out = model.forward_grounding([dict(x, captions=grounding.preprocess_caption(x["captions"])) for x in batch])
    Q = out["pred_logits"].shape[1]
    assert tuple(out["pred_logits"].shape) == (2, Q, 32) and tuple(out["pred_boxes"].shape) == (2, Q, 4)
    prob = out["pred_logits"].sigmoid().cpu()
    assert bool((prob[0, :, 10:] == 0).all()) and bool((prob[1, :, 7:] == 0).all())    # -inf behind each caption's tokens
    assert bool((prob[0, :, :10] > 0).all()) and bool((prob[1, :, :7] > 0).all())
    # thresholds from the model's own output: between the images' score quantiles, so that the twin alone keeps some and drops some
    s = prob.max(dim=2).values
    text_thr = float(prob[prob > 0].quantile(0.5))
    for lo_q, hi_q in ((0.25, 0.75), (0.1, 0.9), (0.0, 1.0)):   # the first pair of quantiles that both images straddle
        lo, hi = max(float(s[i].quantile(lo_q)) for i in range(2)), min(float(s[i].quantile(hi_q)) for i in range(2))
        box_thr = 0.5 * (lo + hi)
        twin_n = grounding.ground_reference(prob, out["pred_boxes"].cpu(), box_thr, text_thr).n_keep.tolist()
        if all(0 < n < Q for n in twin_n):
            break
    assert all(0 < n < Q for n in twin_n), twin_n

    calls = []
    real = grounding.ground
    monkeypatch.setattr(grounding, "ground", lambda *a_, **k: (calls.append(1), real(*a_, **k))[1])
    for order in (0, 1):
        monkeypatch.setattr(zt.Switches, "native_grounding", True)
        got = grounding.predict(model, batch, box_thr, text_thr, order)
        assert len(calls) == 1 + order                          # one call for the batch
        monkeypatch.setattr(zt.Switches, "native_grounding", False)
        want = grounding.predict(model, batch, box_thr, text_thr, order)
        assert len(calls) == 1 + order
        assert len(got) == len(want) == 2
        for (gb, gl, gp), (wb, wl, wp), n in zip(got, want, twin_n):
            assert tuple(gb.shape) == (n, 4) and tuple(gl.shape) == (n,) and len(gp) == n
            assert torch.equal(gb, wb) and torch.equal(gl, wl) and gp == wp
            assert all(isinstance(p, str) for p in gp)
            if order == 1:
                assert bool((gl[:-1] >= gl[1:]).all())
    assert not model.training and len(memo) == 1
