"""Canvas batching on the host (canvas.py): the choice of the canvas, the default set against the ODinW size distribution,
``place_reference`` against the op chain it stands for, and the model's switch on the CPU, where the fallback builds the batch."""
import pytest
import torch

from ziragroundingdino_amd import canvas
from ziragroundingdino_amd.structures import ImageList
from ziragroundingdino_amd.utils import NestedTensor, nested_tensor_from_tensor_list

MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.12, 57.375]


def test_choose_picks_the_smallest_containing_canvas():
    cv = [(128, 128), (96, 128), (64, 256), (256, 64), (32, 512)]
    assert canvas.choose(96, 128, cv) == (96, 128)
    assert canvas.choose(97, 100, cv) == (128, 128)
    assert canvas.choose(1, 1, cv) == (96, 128)                 # the smallest area of all
    assert canvas.choose(10, 200, cv) == (32, 512)              # three canvases of 16384 pixels hold it: the smallest H
    assert canvas.choose(40, 200, cv) == (64, 256)
    assert canvas.choose(200, 10, cv) == (256, 64)
    assert canvas.choose(129, 10, cv) == (256, 64) and canvas.choose(129, 65, cv) is None
    assert canvas.choose(10, 513, cv) is None
    # ties go to the smaller H, whatever the order of the list
    assert canvas.choose(8, 8, [(256, 64), (64, 256)]) == (64, 256) == canvas.choose(8, 8, [(64, 256), (256, 64)])
    top = max(canvas.DEFAULT_CANVASES, key=lambda c: c[0] * c[1])
    assert canvas.choose(top[0] + 1, 32) is None and canvas.choose(32, top[1] + 1) is None
    assert canvas.choose(*top) == top


def test_default_canvases_cover_the_odinw_sizes():
    cv = canvas.DEFAULT_CANVASES
    assert len(cv) <= 12 and len(set(cv)) == len(cv)
    assert all(h % 32 == 0 and w % 32 == 0 for h, w in cv)
    assert max(cv, key=lambda c: c[0] * c[1]) == (1344, 1344)
    for short in range(480, 801, 32):
        for long in range(short, 1334):
            for h, w in ((short, long), (long, short)):
                got = canvas.choose(h, w)
                assert got is not None and got[0] >= h and got[1] >= w, (h, w)
                assert all(H * W >= got[0] * got[1] for H, W in cv if H >= h and W >= w), (h, w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_place_reference_equals_the_op_chain_on_the_batch_maximum(dtype):
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8).to(dtype) for h, w in ((37, 53), (64, 41), (5, 7))]
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    want = nested_tensor_from_tensor_list(ImageList.from_tensors([(x.float() - mean) / std for x in images]))
    tensor, mask = canvas.place_reference(images, (64, 53), MEAN, STD)
    assert tensor.dtype == torch.float32 and mask.dtype == torch.bool
    assert torch.equal(tensor, want.tensors) and torch.equal(mask, want.mask)
    with pytest.raises(ValueError):
        canvas.place_reference(images, (63, 53), MEAN, STD)
    # a larger canvas: the same values in the top-left corner, zeros and a True mask around them
    big, big_mask = canvas.place_reference(images, (96, 64), MEAN, STD)
    assert torch.equal(big[:, :, :64, :53], tensor) and torch.equal(big_mask[:, :64, :53], mask)
    assert not big[:, :, 64:].any() and not big[:, :, :, 53:].any() and big_mask[:, 64:].all() and big_mask[:, :, 53:].all()


def test_supported_declines_on_the_host():
    img = torch.zeros(3, 8, 8)
    assert not canvas.supported([img])          # a CPU tensor
    assert not canvas.supported([])
    with pytest.raises(RuntimeError):
        canvas.place([img], (32, 32), MEAN, STD)


def test_cpu_model_with_canvases_takes_the_fallback(monkeypatch):
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import synthetic_batch

    model = small_model(dev="cpu").eval()
    a = synthetic_batch(1, 64, 96, n_categories=3, boxes_per_image=2, seed=1)[0]
    b = synthetic_batch(1, 80, 72, n_categories=3, boxes_per_image=2, seed=2)[0]
    data = [a, b]
    calls = {"place": 0, "reference": 0}
    real_ref = canvas.place_reference
    monkeypatch.setattr(canvas, "place", lambda *a_, **k: calls.__setitem__("place", calls["place"] + 1))
    monkeypatch.setattr(canvas, "place_reference",
                        lambda *a_, **k: (calls.__setitem__("reference", calls["reference"] + 1), real_ref(*a_, **k))[1])
    assert model.canvas_sizes is None
    model.canvas_sizes = [(96, 128), (128, 128)]
    assert model._graphed_transformer.evict_lru and model._graphed_transformer.max_signatures == 2
    assert model._graphed_backbone.evict_lru and model._graphed_backbone.max_signatures == 2
    with torch.no_grad():
        got = model(data)
    assert calls == {"place": 0, "reference": 1}
    # the existing path on a hand-built NestedTensor of the canvas the two images choose, (96, 128)
    model.canvas_sizes = None
    assert not model._graphed_transformer.evict_lru and model._graphed_transformer.max_signatures == 2
    assert not model._graphed_backbone.evict_lru and model._graphed_backbone.max_signatures == 8
    normed = [model.normalizer(x["image"]) for x in data]
    tensor = torch.zeros(2, 3, 96, 128)
    mask = torch.ones(2, 96, 128, dtype=torch.bool)
    for i, t in enumerate(normed):
        tensor[i, :, :t.shape[1], :t.shape[2]] = t
        mask[i, :t.shape[1], :t.shape[2]] = False
    samples = NestedTensor(tensor, mask)
    with torch.no_grad():
        features, poss = model.run_backbone(samples)
        captions, _ = model._captions(data)
        text_dict, cate, lin = model.encode_text(captions, samples.device)
        out = model.forward_features(features, poss, samples.mask, text_dict, cate, lin, None)
        want = model.postprocess(out["pred_logits"], out["pred_boxes"], data, [(64, 96), (80, 72)])
    assert calls == {"place": 0, "reference": 1}
    assert len(got) == len(want) == 2
    for g_, w_ in zip(got, want):
        gi, wi = g_["instances"], w_["instances"]
        assert gi.image_size == wi.image_size
        assert torch.equal(gi.pred_boxes.tensor, wi.pred_boxes.tensor) and torch.equal(gi.scores, wi.scores)
        assert torch.equal(gi.pred_classes, wi.pred_classes)
    # a batch that no canvas holds takes the path of None
    model.canvas_sizes = [(32, 32)]
    with torch.no_grad():
        res = model(data)
    assert calls == {"place": 0, "reference": 1} and len(res) == 2
