"""Device augmentation on the GPU (csrc/resample.hip): the coefficient tables against the oracle's taps and bounds exactly,
the resampling kernel against the oracle (tests/pillow_oracle.py, pinned to Pillow by tests/golden/resample_pillow.npz) bit for
bit at the smallest shapes that reach each hazard, the refusals, capture and replay, the two-stage chain against Pillow's, and
the mapper in front of ``canvas.place``.  Pillow itself is never imported here."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pillow_oracle  # noqa: E402
from conftest import GOLDEN, load_npz  # noqa: E402

from ziragroundingdino_amd import _lib, augment, canvas  # noqa: E402
from ziragroundingdino_amd.augment import AugmentParams  # noqa: E402

GUARD, SENTINEL = 64, 0xA5
ODINW_EDGES = tuple(range(480, 801, 32))


# ---- part 1: coefficients -------------------------------------------------------------------------------------------------------

def _check_pairs(pairs):
    for lo in range(0, len(pairs), 16):
        part = pairs[lo:lo + 16]
        tables, before, after = augment.device_coefficients(part, "cuda")
        assert (before == 0xFF).all() and (after == 0xFF).all()
        for (n_in, n_out), (bounds, taps) in zip(part, tables):
            want_b, want_t, ksize = pillow_oracle.coefficients(n_in, n_out)
            assert taps.shape == (n_out, ksize), (n_in, n_out)
            assert np.array_equal(bounds, want_b), (n_in, n_out)
            assert np.array_equal(taps, want_t), (n_in, n_out, int((taps != want_t).sum()))


def test_coefficients_equal_oracle_small_sweep():
    """Every in in 1..64 against every out in 1..64 with out >= in / 8."""
    pairs = [(n_in, n_out) for n_in in range(1, 65) for n_out in range(1, 65) if 8 * n_out >= n_in]
    assert len(pairs) > 3500
    _check_pairs(pairs)


def test_coefficients_equal_oracle_odinw_lengths():
    _check_pairs([(n_in, n_out) for n_in in (400, 427, 500, 600, 640, 1024) for n_out in ODINW_EDGES + (1333,)])


# ---- part 2: the kernel ---------------------------------------------------------------------------------------------------------

def _source(h, w, layout, seed):
    """(numpy [h, w, 3], device tensor in ``layout``)."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    t = torch.from_numpy(img).cuda()
    return img, (t if layout == "hwc" else t.permute(2, 0, 1).contiguous())


def _run_guarded(sources, sizes, flips):
    """``augment.resample`` into exact-size buffers between sentinel bytes, the workspace filled with 0xFF beforehand."""
    augment._workspace(torch.device("cuda", torch.cuda.current_device()), 1 << 21).fill_(0xFF)
    bufs = [torch.full((3 * nh * nw + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for nh, nw in sizes]
    outs = [b[GUARD:GUARD + 3 * nh * nw].view(3, nh, nw) for b, (nh, nw) in zip(bufs, sizes)]
    got = augment.resample(sources, sizes, flips, out=outs)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    for b in bufs:
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all()
    return [o.cpu().numpy() for o in outs]


def _want(img, nh, nw, flip=False):
    return pillow_oracle.resize(img[:, ::-1] if flip else img, nh, nw).transpose(2, 0, 1)


HAZARDS = {
    "upscale": (37, 53, 80, 111),
    "downscale": (37, 53, 17, 29),
    "axis_skipped": (64, 48, 64, 20),
    "downscale_8_halo": (33, 200, 5, 25),          # ksize 17; the 5 output rows need all 33 source rows: more than a row tile
    "single_pixel": (5, 5, 1, 1),
    "width_1": (20, 7, 31, 1),
    "width_3": (9, 7, 20, 3),
    "width_5": (12, 11, 7, 5),
    "width_130": (21, 97, 18, 130),                # three column tiles, the last two pixels wide
    "several_row_tiles": (70, 10, 50, 13),
}


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("case", sorted(HAZARDS))
def test_kernel_equals_oracle(case, layout):
    h, w, nh, nw = HAZARDS[case]
    img, src = _source(h, w, layout, seed=len(case))
    for flip in (False, True):
        got = _run_guarded([src], [(nh, nw)], [flip])[0]
        want = _want(img, nh, nw, flip)
        assert np.array_equal(got, want), (case, layout, flip, int((got != want).sum()))


def test_saturated_edges_round_and_clamp():
    """0 / 255 checkerboards: the sums land exactly on the rounding term and on the clamp."""
    img = np.zeros((24, 40, 3), np.uint8)
    img[::2, 1::2] = 255
    img[1::2, ::3, 1] = 255
    src = torch.from_numpy(img).cuda()
    for nh, nw in [(48, 80), (13, 17), (24, 5)]:
        assert np.array_equal(_run_guarded([src], [(nh, nw)], [False])[0], _want(img, nh, nw))


def test_cropped_view_as_source():
    """Non-contiguous views of a larger buffer, both layouts: rows and channel planes of the parent apart."""
    img, hwc = _source(50, 70, "hwc", seed=2)
    chw = hwc.permute(2, 0, 1).contiguous()
    y0, x0, ch, cw = 7, 9, 31, 45
    views = [hwc[y0:y0 + ch, x0:x0 + cw], chw[:, y0:y0 + ch, x0:x0 + cw]]
    assert not any(v.is_contiguous() for v in views)
    crop = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
    got = _run_guarded(views, [(40, 27), (40, 27)], [True, False])
    assert np.array_equal(got[0], _want(crop, 40, 27, True)) and np.array_equal(got[1], _want(crop, 40, 27))


def test_eight_images_of_different_sizes_in_one_launch():
    shapes = [(37, 53, 80, 111), (64, 48, 64, 20), (5, 5, 1, 1), (33, 200, 5, 25), (9, 70, 33, 66), (40, 40, 40, 40),
              (1, 30, 8, 30), (17, 1, 3, 4)]
    pairs = [_source(h, w, "hwc" if i % 2 else "chw", seed=40 + i) for i, (h, w, _, _) in enumerate(shapes)]
    flips = [bool(i % 3 == 0) for i in range(8)]
    got = _run_guarded([p[1] for p in pairs], [(nh, nw) for _, _, nh, nw in shapes], flips)
    for (img, _), (_, _, nh, nw), flip, g in zip(pairs, shapes, flips, got):
        assert np.array_equal(g, _want(img, nh, nw, flip)), (img.shape, nh, nw, flip)


# ---- part 3: behaviour ------------------------------------------------------------------------------------------------------------

def _descs(entries):
    descs = (_lib.ResampleImage * len(entries))()
    for d, (src, dst, h, w, nh, nw) in zip(descs, entries):
        d.src, d.dst, d.h, d.w, d.new_h, d.new_w = src, dst, h, w, nh, nw
        d.stride_c, d.stride_r, d.stride_x = h * w, w, 1
    return descs


def test_refusals():
    lib = _lib.load()
    src = torch.zeros(3 * 64 * 801, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(3 * 64 * 128, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    s, d, p = src.data_ptr(), dst.data_ptr(), ws.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    served = (s, d, 8, 800, 8, 100)                                # downscale 8: served
    n = lib.zira_resample_ws_bytes(_descs([served]), 1)
    assert n == 4 * ((2 + 17) * 100 + (2 + 3) * 8)
    refused = [
        [(s, d, 8, 801, 8, 100)],                                   # downscale 8.01
        [(s, d, 33, 8, 4, 8)],                                      # the other axis
        [(s, d, 4097, 8, 4097, 8)], [(s, d, 8, 8, 8, 4097)],        # sides past 4096
        [(s, d, 0, 8, 4, 8)], [(s, d, 8, 8, 8, 0)],
        [served] * 9,                                               # nine images
    ]
    for entries in refused:
        descs = _descs(entries)
        assert lib.zira_resample_ws_bytes(descs, len(entries)) == 0
        assert lib.zira_resample_coeffs(descs, len(entries), p, ws.numel(), stream) == 1
        assert lib.zira_resample_u8(descs, len(entries), p, ws.numel(), stream) == 1
    ok = _descs([served])
    assert lib.zira_resample_ws_bytes(None, 1) == 0 and lib.zira_resample_ws_bytes(ok, 0) == 0
    assert lib.zira_resample_coeffs(None, 1, p, ws.numel(), stream) == 1
    assert lib.zira_resample_coeffs(ok, 1, None, ws.numel(), stream) == 1
    assert lib.zira_resample_coeffs(ok, 1, p, n - 1, stream) == 1             # workspace too small
    assert lib.zira_resample_u8(ok, 1, None, ws.numel(), stream) == 1
    assert lib.zira_resample_u8(ok, 1, p, n - 1, stream) == 1
    assert lib.zira_resample_u8(_descs([(None, d, 8, 800, 8, 100)]), 1, p, ws.numel(), stream) == 1
    assert lib.zira_resample_u8(_descs([(s, None, 8, 800, 8, 100)]), 1, p, ws.numel(), stream) == 1
    bad = _descs([served])
    bad[0].stride_x = 0
    assert lib.zira_resample_u8(bad, 1, p, ws.numel(), stream) == 1
    torch.cuda.synchronize()
    assert not dst.any()                                            # nothing was launched
    # the Python side: declined batches go to the reference, the served boundary to the kernel
    img = torch.randint(0, 256, (3, 8, 801), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    assert not augment.supported([img], [(8, 100)]) and augment.supported([img[:, :, :800]], [(8, 100)])
    with pytest.raises(RuntimeError):
        augment.resample([img], [(8, 100)])
    got = augment.apply_image([img], [AugmentParams(False, None, None, (8, 100))])[0]
    assert torch.equal(got, augment.resample_reference(img, 8, 100))
    got = augment.resample([img[:, :, :800]], [(8, 100)])[0]
    assert torch.equal(got, augment.resample_reference(img[:, :, :800], 8, 100))


def test_repeatable():
    _, src = _source(45, 61, "hwc", seed=9)
    a = augment.resample([src, src], [(33, 80), (70, 19)], [False, True])
    b = augment.resample([src, src], [(33, 80), (70, 19)], [False, True])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[0], augment.resample_reference(src, 33, 80))
    assert torch.equal(a[1], augment.resample_reference(src, 70, 19, flip=True))


def test_capture_and_replay_on_changed_pixels():
    imgs = [np.random.default_rng(s).integers(0, 256, (37, 53, 3), dtype=np.uint8) for s in (1, 2)]
    static = torch.from_numpy(imgs[0]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        augment.resample([static], [(50, 41)], [True])               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = augment.resample([static, static], [(50, 41), (20, 90)], [True, False])
    for img in (imgs[1], imgs[0]):
        static.copy_(torch.from_numpy(img).cuda())
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), _want(img, 50, 41, True))
        assert np.array_equal(out[1].cpu().numpy(), _want(img, 20, 90))


def test_two_stage_chain_equals_pillow_fixture():
    fx = load_npz(os.path.join(GOLDEN, "resample_pillow.npz"))
    c = [int(v) for v in fx["chain"]]
    p = AugmentParams(bool(c[1]), (c[2], c[3]), tuple(c[4:8]), (c[8], c[9]))
    src = torch.from_numpy(fx["img%d" % c[0]]).cuda()
    assert augment.supported([src], [p.first])
    got = augment.apply_image([src, src.permute(2, 0, 1).contiguous()], [p, p])
    want = fx["chain_out"].transpose(2, 0, 1)
    assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want)
    # and the single resizes of the fixture, Pillow's own bytes
    served = 0
    for j, (i, nh, nw) in enumerate(fx["pairs"]):
        src = torch.from_numpy(fx["img%d" % i]).cuda()
        if not augment.supported([src], [(int(nh), int(nw))]):       # 37 rows into 1, 53 columns into 1: past the factor of 8
            assert src.shape[0] > 8 * nh or src.shape[1] > 8 * nw
            continue
        served += 1
        got = augment.resample([src], [(int(nh), int(nw))])[0]
        assert np.array_equal(got.cpu().numpy(), fx["out%d" % j].transpose(2, 0, 1)), j
    assert served == len(fx["pairs"]) - 2


def test_mapper_into_canvas_place():
    """A minibatch of two, one image through each branch: the mapper's images placed by the kernel = the oracle's images
    placed by the op chain, bit for bit; every resize ran in the kernels."""
    mean, std = [123.675, 116.280, 103.530], [58.395, 57.12, 57.375]
    cfg = augment.AugmentConfig(flip_prob=0.5, short_edges=(48, 56, 64), max_size=96, crop_prob=0.5, crop_short_edges=(40, 50),
                                crop_range=(24, 36))
    imgs = [np.random.default_rng(s).integers(0, 256, hw + (3,), dtype=np.uint8) for s, hw in ((1, (60, 81)), (2, (90, 47)))]
    dicts = [{"image": torch.from_numpy(imgs[0]).cuda(), "boxes": torch.tensor([[5.0, 6.0, 70.0, 50.0]]), "classes": torch.tensor([1])},
             {"image": torch.from_numpy(imgs[1]).cuda().permute(2, 0, 1).contiguous(),
              "boxes": torch.tensor([[1.0, 2.0, 40.0, 80.0], [10.0, 10.0, 11.0, 11.0]]), "classes": torch.tensor([0, 2])}]
    seed = next(s for s in range(100)
                if len({augment.sample_params(h, w, r, True, cfg).crop is None
                        for r in [np.random.default_rng(s)] for h, w in ((60, 81), (90, 47))}) == 2)
    calls = []
    real = augment.resample_reference
    augment.resample_reference = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        out = augment.DeviceMapper(cfg, True, ["cat", "dog", "bird"])(dicts, rng=np.random.default_rng(seed))
    finally:
        augment.resample_reference = real
    assert calls == [] and {o["params"].crop is None for o in out} == {True, False}
    images = [o["image"] for o in out]
    assert canvas.supported(images)
    want = [torch.from_numpy(pillow_oracle.chain(img, o["params"].flip, o["params"].first, o["params"].crop, o["params"].final)
                             .transpose(2, 0, 1).copy()).cuda() for img, o in zip(imgs, out)]
    got_t, got_m = canvas.place(images, (96, 96), mean, std)
    want_t, want_m = canvas.place_reference(want, (96, 96), mean, std)
    assert torch.equal(got_t, want_t) and torch.equal(got_m, want_m)
    for o, d in zip(out, dicts):
        inst = o["instances"]
        assert inst.image_size == o["params"].final == tuple(o["image"].shape[1:]) and o["captions"] == "cat.dog.bird."
        assert inst.gt_boxes.tensor.dtype == torch.float32 and len(inst.gt_boxes) == len(inst.gt_classes) <= len(d["boxes"])
