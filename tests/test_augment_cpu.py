"""Host side of the device augmentation: the numpy oracle against Pillow's recorded (and, where importable, live) outputs,
``augment.resample_reference`` against the oracle, ResizeShortestEdge's size rule, the box transform, the draws and the
mapper's output format -- none of it needs a GPU."""
import os

import numpy as np
import pytest
import torch

import pillow_oracle
from conftest import GOLDEN, load_npz

from ziragroundingdino_amd import augment
from ziragroundingdino_amd.augment import AugmentParams


@pytest.fixture(scope="module")
def fixture():
    return load_npz(os.path.join(GOLDEN, "resample_pillow.npz"))


def _chain_args(fx):
    c = [int(v) for v in fx["chain"]]
    return fx["img%d" % c[0]], bool(c[1]), (c[2], c[3]), tuple(c[4:8]), (c[8], c[9])


# ---- part 1: resampling --------------------------------------------------------------------------------------------------------

def test_oracle_equals_the_pillow_fixture(fixture):
    assert len(fixture["pairs"]) >= 12
    for j, (i, nh, nw) in enumerate(fixture["pairs"]):
        got = pillow_oracle.resize(fixture["img%d" % i], int(nh), int(nw))
        want = fixture["out%d" % j]
        assert got.shape == want.shape == (nh, nw, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want), (j, int((got != want).sum()))
    img, flip, first, crop, final = _chain_args(fixture)
    assert np.array_equal(pillow_oracle.chain(img, flip, first, crop, final), fixture["chain_out"])


def test_oracle_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for h, w, nh, nw in [(37, 53, 80, 111), (37, 53, 17, 29), (64, 48, 64, 20), (33, 200, 5, 25), (5, 5, 1, 1), (30, 40, 97, 130),
                         (48, 64, 48, 65), (1, 9, 4, 2), (61, 7, 8, 56)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
        assert np.array_equal(pillow_oracle.resize(img, nh, nw), want), (h, w, nh, nw)


SHAPES = [(37, 53, 80, 111), (37, 53, 17, 29), (64, 48, 64, 20), (33, 200, 5, 25), (5, 5, 1, 1), (20, 130, 20, 131), (9, 1, 1, 7)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resample_reference_equals_oracle(shape):
    h, w, nh, nw = shape
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    hwc = torch.from_numpy(img)
    chw = hwc.permute(2, 0, 1).contiguous()
    for flip in (False, True):
        want = pillow_oracle.resize(img[:, ::-1] if flip else img, nh, nw).transpose(2, 0, 1)
        for src in (hwc, chw):
            got = augment.resample_reference(src, nh, nw, flip=flip)
            assert got.shape == (3, nh, nw) and got.dtype == torch.uint8 and got.is_contiguous()
            assert np.array_equal(got.numpy(), want), (shape, flip)


def test_coefficients_equal_oracle():
    for n_in, n_out in [(53, 111), (53, 29), (200, 25), (5, 1), (48, 48), (640, 800), (1024, 1333), (427, 480)]:
        bounds, taps, ksize = pillow_oracle.coefficients(n_in, n_out)
        xmin, xmax, got = augment._coefficients(n_in, n_out)
        assert got.shape == (n_out, ksize)
        assert np.array_equal(xmin, bounds[:, 0]) and np.array_equal(xmax, bounds[:, 1]) and np.array_equal(got, taps)


def test_reference_chain_equals_the_pillow_fixture(fixture):
    img, flip, first, crop, final = _chain_args(fixture)
    got = augment.apply_image([torch.from_numpy(img)], [AugmentParams(flip, first, crop, final)])[0]
    assert np.array_equal(got.numpy(), fixture["chain_out"].transpose(2, 0, 1))


# ---- part 2: ResizeShortestEdge's size rule ------------------------------------------------------------------------------------

def test_output_shape_hand_worked():
    assert augment.output_shape(480, 640, 800, 1333) == (800, 1067)        # 640 * 800 / 480 = 1066.67
    assert augment.output_shape(1024, 1024, 800, 1333) == (800, 800)
    assert augment.output_shape(500, 2000, 800, 1333) == (333, 1333)       # 800 x 3200 -> x 1333 / 3200: 333.25 x 1333
    assert augment.output_shape(2000, 500, 800, 1333) == (1333, 333)
    # int(x + 0.5) decides: 333 * 480 / 320 = 499.5 -> 500; truncation would give 499
    assert augment.output_shape(320, 333, 480, 1333) == (480, 500)
    assert augment.output_shape(427, 640, 600) == (600, 899)               # no maximum: 640 * 600 / 427 = 899.30


# ---- part 3: boxes, draws, the mapper -------------------------------------------------------------------------------------------

def test_apply_boxes_hand_worked():
    boxes = torch.tensor([[10.0, 20.0, 50.0, 60.0], [0.0, 0.0, 100.0, 80.0]])
    # scale only: 80 x 100 -> 160 x 150: x * 1.5, y * 2
    got, keep = augment.apply_boxes(boxes, 80, 100, AugmentParams(False, None, None, (160, 150)))
    assert got.dtype == torch.float32 and keep.tolist() == [0, 1]
    assert got.tolist() == [[15.0, 40.0, 75.0, 120.0], [0.0, 0.0, 150.0, 160.0]]
    # flip: x -> 100 - x, corners swapped
    got, keep = augment.apply_boxes(boxes, 80, 100, AugmentParams(True, None, None, (80, 100)))
    assert got.tolist() == [[50.0, 20.0, 90.0, 60.0], [0.0, 0.0, 100.0, 80.0]] and keep.tolist() == [0, 1]
    # flip, x 2, crop (y0 = 30, x0 = 110, 100 x 60), x 0.5: the first box becomes x 50..90 -> 100..180 -> -10..70 -> -5..35 ->
    # clipped to 0..30, y 40..120 -> 10..90 -> 5..45
    p = AugmentParams(True, (160, 200), (30, 110, 100, 60), (50, 30))
    got, keep = augment.apply_boxes(boxes, 80, 100, p)
    assert keep.tolist() == [0, 1]
    assert got.tolist() == [[0.0, 5.0, 30.0, 45.0], [0.0, 0.0, 30.0, 50.0]]
    # a box cropped away (entirely left of the crop) and a box clipped to zero width (it ends on the crop's left edge)
    boxes = torch.tensor([[10.0, 10.0, 30.0, 30.0], [20.0, 10.0, 50.0, 40.0], [40.0, 20.0, 70.0, 50.0]])
    p = AugmentParams(False, (80, 100), (0, 50, 80, 50), (80, 50))
    got, keep = augment.apply_boxes(boxes, 80, 100, p)
    assert keep.tolist() == [2] and got.tolist() == [[0.0, 20.0, 20.0, 50.0]]
    got, keep = augment.apply_boxes(torch.zeros(0, 4), 80, 100, p)
    assert got.shape == (0, 4) and keep.shape == (0,)


def test_sample_params_ranges_and_determinism():
    cfg = augment.ODINW_TRAIN
    assert cfg.short_edges == (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800) and cfg.max_size == 1333
    assert cfg.crop_short_edges == (400, 500, 600) and cfg.crop_range == (384, 600)
    a = [augment.sample_params(427, 640, np.random.default_rng(11)) for _ in range(2)]
    assert a[0] == a[1]
    rng = np.random.default_rng(5)
    seen_flip, seen_crop = set(), set()
    for h, w in [(427, 640), (1024, 1024), (300, 900), (640, 480)] * 25:
        p = augment.sample_params(h, w, rng)
        seen_flip.add(p.flip), seen_crop.add(p.crop is not None)
        ch, cw = h, w
        if p.crop is not None:
            fh, fw = p.first
            assert min(fh, fw) in (400, 500, 600) and p.first == augment.output_shape(h, w, min(fh, fw))
            y0, x0, ch, cw = p.crop
            assert min(fh, 384) <= ch <= min(fh, 600) and min(fw, 384) <= cw <= min(fw, 600)
            assert 0 <= y0 <= fh - ch and 0 <= x0 <= fw - cw
        else:
            assert p.first is None
        assert max(p.final) <= 1333 and p.final in {augment.output_shape(ch, cw, s, 1333) for s in cfg.short_edges}
    assert seen_flip == {False, True} and seen_crop == {False, True}
    # the test configuration draws nothing
    rng = np.random.default_rng(0)
    state = rng.bit_generator.state
    p = augment.sample_params(480, 640, rng, train=False)
    assert p == AugmentParams(False, None, None, (800, 1067)) and rng.bit_generator.state == state


def test_mapper_output_format_on_cpu_tensors():
    g = torch.Generator().manual_seed(0)
    cfg = augment.AugmentConfig(flip_prob=0.5, short_edges=(24, 32), max_size=48, crop_prob=0.5, crop_short_edges=(20, 28),
                                crop_range=(12, 20))
    dicts = [{"image": torch.randint(0, 256, (30, 44, 3), generator=g, dtype=torch.uint8),
              "boxes": torch.tensor([[2.0, 3.0, 40.0, 28.0], [10.0, 5.0, 20.0, 15.0]]), "classes": torch.tensor([1, 0])},
             {"image": torch.randint(0, 256, (3, 40, 26), generator=g, dtype=torch.uint8),
              "boxes": torch.tensor([[1.0, 1.0, 25.0, 39.0]]), "classes": torch.tensor([2])}]
    mapper = augment.DeviceMapper(cfg, True, ["cat", "dog", "bird"], seed=4)
    out = mapper(dicts)
    assert len(out) == 2
    for d, o in zip(dicts, out):
        p = o["params"]
        img = o["image"]
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3 and img.is_contiguous()
        assert tuple(img.shape[1:]) == p.final == o["instances"].image_size
        assert o["captions"] == "cat.dog.bird."
        src = augment.as_chw(d["image"])
        assert (o["height"], o["width"]) == tuple(src.shape[1:])
        inst = o["instances"]
        assert inst.gt_boxes.tensor.dtype == torch.float32 and inst.gt_classes.dtype == torch.int64
        assert len(inst.gt_boxes) == len(inst.gt_classes) <= len(d["boxes"])
        want = pillow_oracle.chain(src.permute(1, 2, 0).numpy(), p.flip, p.first, p.crop, p.final)
        assert np.array_equal(img.numpy(), want.transpose(2, 0, 1))
        boxes, keep = augment.apply_boxes(d["boxes"], src.shape[1], src.shape[2], p)
        assert torch.equal(inst.gt_boxes.tensor, boxes) and torch.equal(inst.gt_classes, d["classes"][keep])
    # the same seed draws the same minibatch; evaluation keeps the boxes out and draws nothing
    again = augment.DeviceMapper(cfg, True, ["cat", "dog", "bird"], seed=4)(dicts)
    assert all(a["params"] == b["params"] and torch.equal(a["image"], b["image"]) for a, b in zip(out, again))
    test = augment.DeviceMapper(augment.AugmentConfig(0.0, (32,), 48), False, ["cat"])(dicts)
    assert [t["params"] for t in test] == [AugmentParams(False, None, None, (32, 47)), AugmentParams(False, None, None, (48, 31))]
    assert all("instances" not in t for t in test)


def test_kernel_path_declines_cpu_tensors():
    img = torch.zeros(3, 8, 8, dtype=torch.uint8)
    assert not augment.supported([img], [(4, 4)])
    with pytest.raises(RuntimeError):
        augment.resample([img], [(4, 4)])
