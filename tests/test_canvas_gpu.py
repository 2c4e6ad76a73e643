"""Canvas batching on the GPU: the placement kernel (csrc/place.hip) against ``canvas.place_reference`` bit for bit, on a side
stream, the model with ``canvas_sizes`` against the existing path on a hand-built canvas, hipGraph replay across a stream of
image sizes, the LRU bound of the graph caches, and the switch being off by default."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import canvas  # noqa: E402
from ziragroundingdino_amd.utils import NestedTensor  # noqa: E402

MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.12, 57.375]


def _images(sizes, dtype, seed=0, offset=0):
    """uint8-valued images [3, h, w] on the GPU; ``offset``: carved out of a flat buffer that many ELEMENTS behind its start
    (contiguous, but the storage offset puts the rows off the 16-byte grid)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in sizes:
        n = 3 * h * w
        flat = torch.randint(0, 256, (n + offset,), generator=g, dtype=torch.uint8).to(dtype).cuda()
        img = flat[offset:offset + n].view(3, h, w)
        assert img.is_contiguous() and img.storage_offset() == offset
        out.append(img)
    return out


CASES = {
    # odd widths: unaligned row starts and tail groups; the second image touches the canvas's bottom edge
    "two_odd": ([(37, 53), (64, 41)], (64, 64), 0),
    "image_is_canvas": ([(32, 64)], (32, 64), 0),
    "one_pixel_image": ([(1, 1), (5, 9), (32, 30)], (32, 32), 0),
    "eight": ([(17, 40), (48, 96), (1, 96), (48, 1), (33, 67), (20, 20), (47, 95), (3, 5)], (48, 96), 0),
    # storage offsets of 1 and 3 elements: 4 / 12 bytes (fp32), 1 / 3 bytes (uint8) -- no multiple of 16
    "offset_1": ([(37, 53), (40, 64)], (64, 64), 1),
    "offset_3": ([(21, 44), (64, 63)], (64, 64), 3),
    # a canvas whose width is no multiple of four: the one-pixel form of the kernel
    "narrow_canvas": ([(37, 53), (20, 30)], (37, 53), 0),
    # several blocks per image, canvas far larger than the images
    "large_canvas": ([(100, 333), (250, 130)], (256, 352), 0),
}


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_place_kernel_equals_reference(case, dtype):
    sizes, cv, offset = CASES[case]
    images = _images(sizes, dtype, seed=len(case), offset=offset)
    if offset:
        assert all(t.data_ptr() % 16 != 0 for t in images)
    assert canvas.supported(images)
    want_t, want_m = canvas.place_reference(images, cv, MEAN, STD)
    got_t, got_m = canvas.place(images, cv, MEAN, STD)
    torch.cuda.synchronize()
    assert got_t.shape == want_t.shape == (len(sizes), 3) + cv and got_t.dtype == torch.float32
    assert got_m.shape == want_m.shape == (len(sizes),) + cv and got_m.dtype == torch.bool
    assert torch.equal(got_m, want_m)
    assert torch.equal(got_t, want_t), float((got_t - want_t).abs().max())
    assert torch.equal(got_m.view(torch.uint8), want_m.view(torch.uint8))    # the bytes are 0 / 1
    if case == "image_is_canvas":
        assert not got_m.any()


def test_fractional_pixels_take_the_same_divide():
    """fp32 sources with arbitrary values (not only 0..255): subtract and divide round as the op chain's."""
    g = torch.Generator().manual_seed(5)
    images = [(torch.randn(3, 33, 47, generator=g) * 300).cuda(), (torch.rand(3, 64, 64, generator=g) * 1e-3).cuda()]
    want_t, want_m = canvas.place_reference(images, (64, 64), MEAN, STD)
    got_t, got_m = canvas.place(images, (64, 64), MEAN, STD)
    assert torch.equal(got_t, want_t) and torch.equal(got_m, want_m)


def test_supported_declines_and_the_fallback_is_equal():
    from test_model_gpu import small_model
    nine = _images([(8 + i, 20 - i) for i in range(9)], torch.float32)
    assert canvas.supported(nine[:8]) and not canvas.supported(nine)
    wide = _images([(30, 80)], torch.float32)[0]
    narrowed = wide[:, :, 3:56]                                  # a view: rows 80 apart, 53 wide
    assert not narrowed.is_contiguous()
    other = _images([(40, 41)], torch.float32, seed=1)[0]
    assert not canvas.supported([narrowed, other]) and canvas.supported([narrowed.contiguous(), other])
    assert not canvas.supported([other.double()]) and not canvas.supported([other.half()])
    assert not canvas.supported([other[:2].contiguous()]) and not canvas.supported([other[None]])
    assert not canvas.supported([other.cpu()]) and not canvas.supported([other, other.to(torch.uint8)])
    with pytest.raises(RuntimeError):
        canvas.place(nine, (32, 32), MEAN, STD)
    with pytest.raises(ValueError):
        canvas.place([other], (40, 40), MEAN, STD)               # does not fit
    # the model falls back to the op chain on the canvas for both, with the result the kernel gives where it serves
    model = small_model()
    model.canvas_sizes = [(64, 64)]
    data = lambda imgs: [{"image": t} for t in imgs]
    _, fb = model._canvas_batch(data([narrowed, other]))
    _, kn = model._canvas_batch(data([narrowed.contiguous(), other]))
    assert torch.equal(fb.tensors, kn.tensors) and torch.equal(fb.mask, kn.mask) and not fb.no_padding
    model.canvas_sizes = [(32, 32)]
    imgs9, fb9 = model._canvas_batch(data(nine))
    _, kn8 = model._canvas_batch(data(nine[:8]))
    assert fb9.tensors.shape == (9, 3, 32, 32) and imgs9.image_sizes == [(8 + i, 20 - i) for i in range(9)]
    assert torch.equal(fb9.tensors[:8], kn8.tensors) and torch.equal(fb9.mask[:8], kn8.mask)
    # no_padding: only when every image IS the canvas
    full = _images([(32, 32), (32, 32)], torch.float32)
    assert model._canvas_batch(data(full))[1].no_padding
    assert not model._canvas_batch(data([full[0], nine[0]]))[1].no_padding


def test_place_on_a_side_stream():
    images = _images([(37, 53), (64, 41)], torch.uint8, seed=3)
    want_t, want_m = canvas.place_reference(images, (64, 64), MEAN, STD)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_t, got_m = canvas.place(images, (64, 64), MEAN, STD)
    torch.cuda.current_stream().wait_stream(side)
    got_t.record_stream(torch.cuda.current_stream())
    got_m.record_stream(torch.cuda.current_stream())
    assert torch.equal(got_t, want_t) and torch.equal(got_m, want_m)


# ---- the model ------------------------------------------------------------------------------------------------------------------

CANVASES = [(96, 128), (128, 128)]


def _batch(sizes, seed):
    from ziragroundingdino_amd.train import synthetic_batch
    return [synthetic_batch(1, h, w, n_categories=4, boxes_per_image=3, seed=seed + i, device="cuda")[0]
            for i, (h, w) in enumerate(sizes)]


def _by_hand(model, data, cv):
    """The existing path fed a hand-built NestedTensor of the canvas, through run_backbone + forward_features."""
    normed = [model.normalizer(x["image"].to(model.device)) for x in data]
    tensor = torch.zeros(len(data), 3, *cv, device="cuda")
    mask = torch.ones(len(data), *cv, dtype=torch.bool, device="cuda")
    for i, t in enumerate(normed):
        tensor[i, :, :t.shape[1], :t.shape[2]] = t
        mask[i, :t.shape[1], :t.shape[2]] = False
    samples = NestedTensor(tensor, mask)
    captions, names_list = model._captions(data)
    finish_text, cate = model.encode_text(captions, samples.device, defer=True)
    targets = None
    if model.training:
        targets = model.prepare_targets([x["instances"].to(model.device) for x in data], cate, names_list)
    features, poss = model.run_backbone(samples)
    text_dict, cate, lin = finish_text()
    out = model.forward_features(features, poss, samples.mask, text_dict, cate, lin, targets, no_padding=False)
    if model.training:
        return out
    sizes = [tuple(x["image"].shape[-2:]) for x in data]
    return model.postprocess(out["pred_logits"], out["pred_boxes"], data, sizes)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_model_on_a_canvas_equals_the_hand_built_canvas(training):
    """Same shapes and kernels on both sides: the losses (training) and the detections (eval) bit for bit."""
    from test_model_gpu import small_model
    model = small_model()
    model.before_train()
    model.train(training)
    data = _batch([(80, 112), (96, 72)], seed=1)             # batch maximum (96, 112) -> canvas (96, 128)
    placed = []
    real = canvas.place
    model.canvas_sizes = CANVASES
    try:
        canvas.place = lambda *a, **k: (placed.append(tuple(a[1])), real(*a, **k))[1]
        with torch.set_grad_enabled(training):
            got = model(data)
    finally:
        canvas.place = real
    assert placed == [(96, 128)]
    model.canvas_sizes = None
    with torch.set_grad_enabled(training):
        want = _by_hand(model, data, (96, 128))
    torch.cuda.synchronize()
    if training:
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
    else:
        assert len(got) == len(want) == 2
        for g_, w_ in zip(got, want):
            gi, wi = g_["instances"], w_["instances"]
            assert gi.image_size == wi.image_size and len(gi) == len(wi)
            assert torch.equal(gi.pred_boxes.tensor, wi.pred_boxes.tensor)
            assert torch.equal(gi.scores, wi.scores) and torch.equal(gi.pred_classes, wi.pred_classes)


def _image_signatures(graphed):
    return {key[0][0] for key in graphed._cache}              # (shape, dtype, device) of the image tensor


def test_replay_across_sizes(monkeypatch):
    """Six minibatches, four distinct batch maxima, two canvases: two sets of graphs, nothing eager, no capture after both
    canvases have been met, and every step's losses those of the same stream launched eagerly on the same canvases."""
    from test_model_gpu import small_model
    from ziragroundingdino_amd import graphs as zg
    from ziragroundingdino_amd.train import ZiraTrainer

    a1, a2 = _batch([(80, 112), (96, 72)], seed=1), _batch([(90, 128), (64, 100)], seed=3)      # -> (96, 128)
    b1, b2 = _batch([(120, 100), (100, 128)], seed=5), _batch([(128, 90), (97, 60)], seed=7)    # -> (128, 128)
    stream = [a1, b1, a2, b2, a1, b2]
    maxima = {(max(x["image"].shape[1] for x in d), max(x["image"].shape[2] for x in d)) for d in stream}
    assert len(maxima) == 4 and {canvas.choose(h, w, CANVASES) for h, w in maxima} == set(CANVASES)

    captures = []
    real_graph = zg._graph
    monkeypatch.setattr(zg, "_graph", lambda *a, **k: (captures.append(1), real_graph(*a, **k))[1])

    def run(graphs):
        model = small_model().train()
        model.canvas_sizes = CANVASES
        model.use_transformer_graph = model.use_frontend_graphs = graphs
        trainer = ZiraTrainer(model)
        losses, caps = [], []
        for i, data in enumerate(stream):
            n = len(captures)
            nxt = stream[i + 1] if graphs and i + 1 < len(stream) else None    # (the next front end prefetched, on its canvas)
            out = trainer.run_step(data, next_data=nxt)
            losses.append(float(sum(out.values())))
            caps.append(len(captures) - n)
        torch.cuda.synchronize()
        return model, losses, caps

    model, graphed, caps = run(True)
    gt = model._graphed_transformer
    assert len(gt._cache) == 2 and gt._eager_keys == set()
    assert all(all(e["layers"]) and e["decode"] is not None for e in gt._cache.values())
    assert _image_signatures(model._graphed_backbone) == {((2, 3) + cv, torch.float32, 0) for cv in CANVASES}
    assert len(model._graphed_backbone._cache) == 2
    assert caps[0] > 0 and caps[1] > 0 and caps[2:] == [0, 0, 0, 0], caps
    _, eager, caps_e = run(False)
    assert caps_e == [0] * 6
    assert all(torch.isfinite(torch.tensor(graphed)))
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (eager, graphed)


def test_lru_at_the_cap():
    """Three canvases under a cap of two, stream A B C A: every step replays (C takes A's place, A then B's), the caches
    never hold more than two sets, and the recaptured A computes what the first A computed (lr = 0: same weights)."""
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import ZiraTrainer

    three = CANVASES + [(128, 160)]
    a, b, c = _batch([(80, 112), (96, 72)], seed=1), _batch([(120, 100), (100, 128)], seed=5), _batch([(128, 140), (70, 160)], seed=9)
    model = small_model().train()
    model.canvas_sizes = three
    gt, gb = model._graphed_transformer, model._graphed_backbone
    assert gt.max_signatures == gb.max_signatures == 3 and gt.evict_lru and gb.evict_lru
    gt.max_signatures = gb.max_signatures = 2
    eager_forwards = []
    real_forward = model.transformer.forward
    model.transformer.forward = lambda *a_, **k: (eager_forwards.append(1), real_forward(*a_, **k))[1]
    trainer = ZiraTrainer(model, lr=0.0)
    outs = []
    for data, cv in ((a, three[0]), (b, three[1]), (c, three[2]), (a, three[0])):
        outs.append(trainer.run_step(data))
        assert 1 <= len(gt._cache) <= 2 and 1 <= len(gb._cache) <= 2
        assert ((2, 3) + cv, torch.float32, 0) in _image_signatures(gb)          # this step's front end came from a graph
        newest = list(gt._cache.values())[-1]
        assert all(newest["layers"]) and newest["decode"] is not None
    torch.cuda.synchronize()
    assert eager_forwards == [] and gt._eager_keys == set()
    assert _image_signatures(gb) == {((2, 3) + three[2], torch.float32, 0), ((2, 3) + three[0], torch.float32, 0)}
    assert set(outs[0]) == set(outs[3])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[3][k]), (k, float(outs[0][k]), float(outs[3][k]))


def test_switch_off_never_places(monkeypatch):
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import ZiraTrainer

    calls = []
    for name in ("place", "place_reference", "choose"):
        monkeypatch.setattr(canvas, name, lambda *a, _n=name, **k: calls.append(_n))
    model = small_model().train()
    assert model.canvas_sizes is None
    assert not model._graphed_transformer.evict_lru and model._graphed_transformer.max_signatures == 2
    assert not model._graphed_backbone.evict_lru and model._graphed_backbone.max_signatures == 8
    trainer = ZiraTrainer(model)
    data = _batch([(80, 112), (96, 72)], seed=1)
    trainer.run_step(data, next_data=data)
    out = trainer.run_step(data)
    assert all(torch.isfinite(v) for v in out.values())
    model.eval()
    with torch.no_grad():
        assert len(model(data)) == 2
    assert calls == []
