"""Device-side training augmentation: the reference's data mapper (detectron2 ``RandomFlip`` -> ``ResizeShortestEdge``, and
on half of the images ``RandomFlip`` -> ``ResizeShortestEdge`` -> ``RandomCrop`` -> ``ResizeShortestEdge``) from decoded
uint8 images to the ``[3, h, w]`` uint8 tensors ``canvas.place`` and ``preprocess_image`` take.

The resize is Pillow's bilinear ``Image.resize`` of a uint8 image (what detectron2's ``ResizeTransform`` calls), bit for bit:
``resample`` runs it on the GPU (csrc/resample.hip: one launch for the coefficient tables, one for a whole minibatch of
differently sized images, flip and crop folded into the source descriptor), ``resample_reference`` is the same arithmetic in
integer torch on any device, for CPU tensors, for what the kernel declines (``supported``) and for the tests.  The random
draws come from the ``numpy.random.Generator`` handed in, in the order ``sample_params`` documents; the reference's global
random stream is not reproduced.  Nothing in the package calls this module by default.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .structures import Boxes, Instances

MAX_IMAGES = _lib.RESAMPLE_MAX_IMAGES
MAX_SIDE = _lib.RESAMPLE_MAX_SIDE
PRECISION_BITS = 22
_WS = {}


@dataclass(frozen=True)
class AugmentConfig:
    """One mapper configuration.  ``crop_*`` None: no crop branch."""
    flip_prob: float
    short_edges: Tuple[int, ...]
    max_size: int
    crop_prob: float = 0.0
    crop_short_edges: Optional[Tuple[int, ...]] = None
    crop_range: Optional[Tuple[int, int]] = None           # RandomCrop(crop_type="absolute_range")


# the values of the reference's ODinW configs (configs/common/data/odinw_*/*.py)
ODINW_TRAIN = AugmentConfig(flip_prob=0.5, short_edges=tuple(range(480, 801, 32)), max_size=1333, crop_prob=0.5,
                            crop_short_edges=(400, 500, 600), crop_range=(384, 600))
ODINW_TEST = AugmentConfig(flip_prob=0.0, short_edges=(800,), max_size=1333)


@dataclass(frozen=True)
class AugmentParams:
    """What was drawn for one image: sizes are (h, w), ``crop`` is (y0, x0, ch, cw) inside the ``first`` resize's output."""
    flip: bool
    first: Optional[Tuple[int, int]]
    crop: Optional[Tuple[int, int, int, int]]
    final: Tuple[int, int]


def output_shape(h, w, size, max_size=None):
    """detectron2 ``ResizeShortestEdge.get_output_shape``: the short side becomes ``size``, the other keeps the ratio; if the
    longer result exceeds ``max_size`` both shrink by ``max_size / longer``; each side is then ``int(x + 0.5)``."""
    scale = size * 1.0 / min(h, w)
    if h < w:
        new_h, new_w = size, scale * w
    else:
        new_h, new_w = scale * h, size
    if max_size is not None and max(new_h, new_w) > max_size:
        scale = max_size * 1.0 / max(new_h, new_w)
        new_h, new_w = new_h * scale, new_w * scale
    return int(new_h + 0.5), int(new_w + 0.5)


def sample_params(h, w, rng, train=True, config=None):
    """Draws one image's parameters from ``rng`` (a ``numpy.random.Generator``), in this order:
      1. ``rng.random()``: the crop branch where it is < ``crop_prob`` (only drawn if the configuration has one);
      2. ``rng.random()``: flip where it is < ``flip_prob`` (only drawn if ``flip_prob`` > 0);
      3. crop branch only: ``rng.choice(crop_short_edges)`` for the first resize (no maximum), then on its output (h', w')
         ``ch = rng.integers(min(h', lo), min(h', hi) + 1)``, ``cw`` likewise from w', ``y0 = rng.integers(0, h' - ch + 1)``,
         ``x0 = rng.integers(0, w' - cw + 1)``;
      4. ``rng.choice(short_edges)`` for the final resize (only drawn if there is more than one).
    ``train=False`` with no ``config`` is ``ODINW_TEST``, which draws nothing."""
    if config is None:
        config = ODINW_TRAIN if train else ODINW_TEST
    crop_branch = config.crop_range is not None and float(rng.random()) < config.crop_prob
    flip = config.flip_prob > 0 and float(rng.random()) < config.flip_prob
    first = crop = None
    ch, cw = h, w
    if crop_branch:
        first = output_shape(h, w, int(rng.choice(config.crop_short_edges)))
        lo, hi = config.crop_range
        ch = int(rng.integers(min(first[0], lo), min(first[0], hi) + 1))
        cw = int(rng.integers(min(first[1], lo), min(first[1], hi) + 1))
        y0 = int(rng.integers(0, first[0] - ch + 1))
        x0 = int(rng.integers(0, first[1] - cw + 1))
        crop = (y0, x0, ch, cw)
    size = config.short_edges[0] if len(config.short_edges) == 1 else int(rng.choice(config.short_edges))
    return AugmentParams(bool(flip), first, crop, output_shape(ch, cw, size, config.max_size))


# ---- the resampling arithmetic on any device ----------------------------------------------------------------------------------

def _coefficients(n_in, n_out):
    """(xmin [n_out], xmax [n_out], taps [n_out, ksize] int64) of one axis: float64 numpy, one rounding per operation."""
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), float(n_in)).astype(np.int64) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < xmax[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(n_out, np.float64)
    for j in range(ksize):                                   # the sum in index order (the zeros behind xmax change nothing)
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    taps = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int64)
    return xmin, xmax, taps


def _pass_last_dim(img, n_out):
    """One pass along the last dimension of an int64 tensor [..., n_in] -> [..., n_out], values 0..255."""
    n_in = img.shape[-1]
    xmin, _, taps = _coefficients(n_in, n_out)
    dev = img.device
    xmin_t, taps_t = torch.from_numpy(xmin).to(dev), torch.from_numpy(taps).to(dev)
    acc = torch.full(img.shape[:-1] + (n_out,), 1 << (PRECISION_BITS - 1), dtype=torch.int64, device=dev)
    for j in range(taps.shape[1]):                           # taps behind xmax are zero: the clamped index reads a valid pixel
        acc += img.index_select(-1, (xmin_t + j).clamp_(max=n_in - 1)) * taps_t[:, j]
    return (acc >> PRECISION_BITS).clamp_(0, 255)


def as_chw(image):
    """A ``[3, H, W]`` view of a uint8 image given as ``[H, W, 3]`` (last dimension 3, first not) or ``[3, H, W]``."""
    if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3):
        raise ValueError("an image is a uint8 tensor [H, W, 3] or [3, H, W]")
    if image.shape[2] == 3 and image.shape[0] != 3:
        return image.permute(2, 0, 1)
    if image.shape[0] != 3:
        raise ValueError("an image is a uint8 tensor [H, W, 3] or [3, H, W], got %s" % (tuple(image.shape),))
    return image


def resample_reference(image, new_h, new_w, flip=False):
    """Pillow's bilinear resize of a uint8 image to ``[3, new_h, new_w]`` (contiguous uint8, the image's device), the columns
    read right to left where ``flip``: horizontal pass first into uint8, then the vertical pass; an unchanged axis is skipped."""
    img = as_chw(image)
    if flip:
        img = img.flip(2)
    _, h, w = img.shape
    img = img.to(torch.int64)
    if new_w != w:
        img = _pass_last_dim(img, int(new_w))
    if new_h != h:
        img = _pass_last_dim(img.transpose(1, 2), int(new_h)).transpose(1, 2)
    return img.to(torch.uint8).contiguous()


# ---- the kernel path ------------------------------------------------------------------------------------------------------------

def supported(images, sizes) -> bool:
    """True where ``resample`` runs the kernels: 1..8 uint8 images on one GPU, every side (source and output) in 1..4096 and no
    axis shrunk by more than 8."""
    images, sizes = list(images), list(sizes)
    if not 1 <= len(images) <= MAX_IMAGES or len(sizes) != len(images):
        return False
    for t, (nh, nw) in zip(images, sizes):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.device == images[0].device):
            return False
        if not ((t.shape[2] == 3 and t.shape[0] != 3) or t.shape[0] == 3):
            return False
        _, h, w = as_chw(t).shape
        if not all(1 <= v <= MAX_SIDE for v in (h, w, nh, nw)) or h > 8 * nh or w > 8 * nw:
            return False
        if min(as_chw(t).stride()) < 1:
            return False
    return True


def _workspace(dev, n_bytes):
    """Kernel scratch, cached and grow-only per (device, stream); left to the graph's own pool while a stream is captured."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < n_bytes:
        ws = _WS[key] = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    return ws


def descriptors(images, sizes, flips, outputs):
    """The ``zira_resample_image`` array of a batch (``outputs``: None where only sizes matter)."""
    descs = (_lib.ResampleImage * len(images))()
    for i, (d, t, (nh, nw)) in enumerate(zip(descs, images, sizes)):
        v = as_chw(t)
        d.src, d.dst = v.data_ptr(), (outputs[i].data_ptr() if outputs is not None else None)
        d.stride_c, d.stride_r, d.stride_x = v.stride()
        d.h, d.w, d.new_h, d.new_w, d.flip = v.shape[1], v.shape[2], int(nh), int(nw), int(bool(flips[i]))
    return descs


def resample(images, sizes, flips=None, out=None):
    """A list of contiguous ``[3, new_h, new_w]`` uint8 tensors (``out`` where given), ``resample_reference`` of each image bit
    for bit, in two launches on the current stream (coefficient tables, then the whole batch).  Capturable: sizes, strides and
    pointers travel in the kernels' argument structs, nothing is uploaded and the host never waits."""
    images, sizes = list(images), [(int(a), int(b)) for a, b in sizes]
    flips = [False] * len(images) if flips is None else list(flips)
    if not supported(images, sizes) or len(flips) != len(images):
        raise RuntimeError("zira_resample_u8 does not serve these images (see augment.supported)")
    lib = _lib.load()
    dev = images[0].device
    with torch.cuda.device(dev):
        outputs = [torch.empty((3, nh, nw), dtype=torch.uint8, device=dev) for nh, nw in sizes] if out is None else list(out)
        if len(outputs) != len(images) or not all(o.dtype == torch.uint8 and o.device == dev and o.is_contiguous()
                                                  and tuple(o.shape) == (3, nh, nw) for o, (nh, nw) in zip(outputs, sizes)):
            raise ValueError("out: one contiguous uint8 [3, new_h, new_w] tensor per image, on the images' device")
        descs = descriptors(images, sizes, flips, outputs)
        n_bytes = lib.zira_resample_ws_bytes(descs, len(images))
        if n_bytes == 0:
            raise RuntimeError("zira_resample_ws_bytes declined a batch that augment.supported accepted")
        ws = _workspace(dev, n_bytes)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.zira_resample_coeffs(descs, len(images), ws.data_ptr(), n_bytes, stream)
        if rc != 0:
            raise RuntimeError("zira_resample_coeffs failed: hipError %d" % rc)
        rc = lib.zira_resample_u8(descs, len(images), ws.data_ptr(), n_bytes, stream)
        if rc != 0:
            raise RuntimeError("zira_resample_u8 failed: hipError %d" % rc)
    return outputs


def device_coefficients(pairs, device):
    """[(bounds [out, 2], taps [out, ksize])] as int32 numpy arrays for up to 16 (in, out) length pairs, as ONE launch of
    ``zira_resample_coeffs`` writes them into a workspace filled with 0xFF beforehand, plus the 64 guard bytes on either side
    of the workspace as they are afterwards.  For tests and for looking at the tables; the training path never reads them back."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    padded = pairs + [(1, 1)] * (len(pairs) % 2)
    descs = (_lib.ResampleImage * (len(padded) // 2))()
    for d, (w, nw), (h, nh) in zip(descs, padded[0::2], padded[1::2]):
        d.w, d.new_w, d.h, d.new_h = w, nw, h, nh
        d.stride_c = d.stride_r = d.stride_x = 1
    lib = _lib.load()
    n_bytes = lib.zira_resample_ws_bytes(descs, len(descs))
    if n_bytes == 0:
        raise RuntimeError("zira_resample_coeffs does not serve these lengths")
    guard = 64
    with torch.cuda.device(device):
        buf = torch.full((n_bytes + 2 * guard,), 0xFF, dtype=torch.uint8, device=device)
        rc = lib.zira_resample_coeffs(descs, len(descs), buf.data_ptr() + guard, n_bytes, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_resample_coeffs failed: hipError %d" % rc)
    host = buf.cpu().numpy()
    table = host[guard:guard + n_bytes].view(np.int32)
    out, at = [], 0
    for n_in, n_out in padded:
        ksize = (1 if n_in <= n_out else -(-n_in // n_out)) * 2 + 1
        bounds = table[at:at + 2 * n_out].reshape(n_out, 2)
        at += 2 * n_out
        out.append((bounds, table[at:at + ksize * n_out].reshape(n_out, ksize)))
        at += ksize * n_out
    assert at * 4 == n_bytes
    return out[:len(pairs)], host[:guard], host[guard + n_bytes:]


def _resample_any(images, sizes, flips):
    if supported(images, sizes):
        return resample(images, sizes, flips)
    return [resample_reference(t, nh, nw, f) for t, (nh, nw), f in zip(images, sizes, flips)]


def apply_image(images, params):
    """The one- or two-stage chain for a minibatch: images that drew the crop branch are flipped and resized to ``first`` in one
    launch, then every image -- the others flipped here, the cropped ones as a view of the first stage's output -- is resized to
    ``final`` in a second one.  Returns the ``[3, h, w]`` uint8 tensors."""
    images, params = list(images), list(params)
    if len(images) != len(params):
        raise ValueError("one AugmentParams per image")
    sources, flips = [as_chw(t) for t in images], [p.flip for p in params]
    staged = [i for i, p in enumerate(params) if p.first is not None]
    for lo in range(0, len(staged), MAX_IMAGES):
        part = staged[lo:lo + MAX_IMAGES]
        firsts = _resample_any([sources[i] for i in part], [params[i].first for i in part], [flips[i] for i in part])
        for i, t in zip(part, firsts):
            sources[i], flips[i] = t, False
    for i, p in enumerate(params):
        if p.crop is not None:
            y0, x0, ch, cw = p.crop
            sources[i] = sources[i][:, y0:y0 + ch, x0:x0 + cw]
    out = []
    for lo in range(0, len(images), MAX_IMAGES):
        hi = lo + MAX_IMAGES
        out += _resample_any(sources[lo:hi], [p.final for p in params[lo:hi]], flips[lo:hi])
    return out


# ---- boxes ------------------------------------------------------------------------------------------------------------------------

def apply_boxes(boxes_xyxy, h, w, params):
    """The boxes of an ``h x w`` image through the same chain, in float64 on the host as detectron2 does: flip (x -> w - x, the
    corners swapped back into order), scale by new_w / w and new_h / h, subtract the crop origin, scale again, clip to the final
    size, drop boxes whose width or height is <= 1e-5, cast to float32.  Returns (boxes [K, 4] float32, kept indices [K] int64)."""
    b = np.asarray(torch.as_tensor(boxes_xyxy).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4).copy()
    if params.flip:
        b[:, [0, 2]] = w - b[:, [2, 0]]
    ch, cw = h, w
    if params.first is not None:
        b[:, 0::2] = b[:, 0::2] * (params.first[1] * 1.0 / w)
        b[:, 1::2] = b[:, 1::2] * (params.first[0] * 1.0 / h)
        ch, cw = params.first
    if params.crop is not None:
        y0, x0, ch, cw = params.crop
        b[:, 0::2] -= x0
        b[:, 1::2] -= y0
    new_h, new_w = params.final
    b[:, 0::2] = b[:, 0::2] * (new_w * 1.0 / cw)
    b[:, 1::2] = b[:, 1::2] * (new_h * 1.0 / ch)
    b = np.minimum(b.clip(min=0), np.array([new_w, new_h, new_w, new_h], np.float64))
    out = torch.from_numpy(b).to(torch.float32)
    keep = torch.nonzero(((out[:, 2] - out[:, 0]) > 1e-5) & ((out[:, 3] - out[:, 1]) > 1e-5)).flatten()
    return out[keep], keep


# ---- the mapper ---------------------------------------------------------------------------------------------------------------------

class DeviceMapper:
    """A list of dataset dicts -> the ``batched_inputs`` of ``GroundingDINO.forward`` / ``ZiraTrainer.run_step``.

    Each dict holds ``image`` (uint8 ``[H, W, 3]`` or ``[3, H, W]``, on the device the resize should run on), and in training
    ``boxes`` (xyxy, ``[N, 4]``) and ``classes`` (``[N]``).  Each result holds ``image`` (``[3, h, w]`` uint8, same device),
    ``captions`` (``".".join(categories_names) + "."``), ``height`` / ``width`` (the original size), ``params`` and in training
    ``instances`` (the transformed boxes as float32 ``gt_boxes``, ``gt_classes`` of the boxes kept, on the host like the
    reference mapper's).  A minibatch of up to eight costs at most two resample and two coefficient launches."""

    def __init__(self, config=None, train=True, categories_names=(), seed=0):
        self.config = config if config is not None else (ODINW_TRAIN if train else ODINW_TEST)
        self.train = bool(train)
        self.categories_names = list(categories_names)
        self.caption = ".".join(self.categories_names) + "."
        self.rng = np.random.default_rng(seed)

    def __call__(self, dataset_dicts, rng=None):
        rng = self.rng if rng is None else rng
        dataset_dicts = list(dataset_dicts)
        views = [as_chw(d["image"]) for d in dataset_dicts]
        params = [sample_params(v.shape[1], v.shape[2], rng, self.train, self.config) for v in views]
        images = apply_image(views, params)
        out = []
        for d, v, p, img in zip(dataset_dicts, views, params, images):
            h, w = int(v.shape[1]), int(v.shape[2])
            item = {"image": img, "captions": self.caption, "height": d.get("height", h), "width": d.get("width", w), "params": p}
            if self.train:
                boxes, keep = apply_boxes(d["boxes"], h, w, p)
                classes = torch.as_tensor(d["classes"]).detach().cpu().to(torch.int64).reshape(-1)[keep]
                item["instances"] = Instances(p.final, gt_boxes=Boxes(boxes), gt_classes=classes)
            out.append(item)
        return out
