"""Canvas batching: a minibatch of differently sized images lands in one of a few FIXED batch sizes ("canvases").

hipGraph replay is keyed on exact tensor shapes (graphs.py), and an ODinW task draws every image from
``ResizeShortestEdge(480 ... 800 step 32, max 1333)`` plus a random crop: padded to its own maximum, a minibatch of two has a
new shape almost every step and leaves the graphs after the first few.  The padding masks carry arbitrary padding, so the batch
can be padded a little further, to the smallest canvas that holds it, and every step replays.

``place`` builds the batch in one launch (csrc/place.hip: normalise, place, zero the rest, write the mask; every output element
written once) instead of the op chain ``preprocess_image`` -> ``ImageList.from_tensors`` -> ``nested_tensor_from_tensor_list``
(per image a copy, a subtract, a divide, a slice copy and a mask slice write, and two fills per batch); ``place_reference`` is
that op chain on a canvas, for what ``supported`` declines and for the tests.  Off by default: ``GroundingDINO.canvas_sizes``.
"""
import torch

from . import _lib

# (H, W), both multiples of 32 (the backbone's total stride), the largest holds every batch of the distribution (both sides
# <= 1333).  The other eleven: greedy choice, one canvas at a time, of the set that minimises the mean canvas / batch-max pixel
# ratio over 20 000 simulated minibatches of two (scripts/canvas_stream.py --pick: landscape, portrait and square originals,
# half of them through the crop branch of the reference's mapper); 1.21 on that stream, profiles/canvas_stream.json for the
# measured one.
DEFAULT_CANVASES = (
    (640, 768), (736, 864), (768, 736), (768, 1024), (800, 928), (800, 1344),
    (864, 768), (864, 1088), (1024, 800), (1088, 1216), (1216, 864), (1344, 1344),
)
MAX_IMAGES = _lib.PLACE_MAX_IMAGES
_STATS = {}


def choose(h, w, canvases=DEFAULT_CANVASES):
    """The smallest-area canvas with H >= h and W >= w (ties: the smaller H); None if none fits."""
    best = None
    for H, W in canvases:
        if H >= h and W >= w and (best is None or (H * W, H) < (best[0] * best[1], best[0])):
            best = (int(H), int(W))
    return best


def supported(images) -> bool:
    """True where ``place`` runs the kernel: 1..8 contiguous [3, h, w] uint8 / float32 tensors of one dtype on one GPU."""
    images = list(images)
    if not 1 <= len(images) <= MAX_IMAGES:
        return False
    first = images[0]
    if not (torch.is_tensor(first) and first.is_cuda and first.dtype in (torch.uint8, torch.float32)):
        return False
    return all(torch.is_tensor(t) and t.device == first.device and t.dtype == first.dtype and t.dim() == 3
               and t.shape[0] == 3 and t.shape[1] >= 1 and t.shape[2] >= 1 and t.is_contiguous() for t in images)


def _check(images, canvas):
    H, W = int(canvas[0]), int(canvas[1])
    for t in images:
        if t.dim() != 3 or t.shape[1] > H or t.shape[2] > W:
            raise ValueError("image %s does not fit canvas %s" % (tuple(t.shape), (H, W)))
    return H, W


def _stats(mean, std, device):
    """mean / std as [C, 1, 1] fp32 tensors on ``device``, uploaded once (a host list -> device tensor is a blocking copy)."""
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std), str(device))
    cached = _STATS.get(key)
    if cached is None:
        cached = _STATS[key] = (torch.tensor(key[0], dtype=torch.float32).view(-1, 1, 1).to(device),
                                torch.tensor(key[1], dtype=torch.float32).view(-1, 1, 1).to(device))
    return cached


def place_reference(images, canvas, mean, std):
    """The op chain on a canvas: (tensor [B, C, H, W] fp32 = ``(x.float() - mean) / std`` in each image's top-left rectangle and
    zero elsewhere, mask [B, H, W] bool, True outside the rectangle).  Any device, any channel count."""
    images = list(images)
    H, W = _check(images, canvas)
    dev = images[0].device
    m, s = _stats(mean, std, dev)
    tensor = torch.zeros((len(images), images[0].shape[0], H, W), dtype=torch.float32, device=dev)
    mask = torch.ones((len(images), H, W), dtype=torch.bool, device=dev)
    for img, pad_img, pad_mask in zip(images, tensor, mask):
        h, w = img.shape[1], img.shape[2]
        pad_img[:, :h, :w].copy_((img.float() - m) / s)
        pad_mask[:h, :w] = False
    return tensor, mask


def place(images, canvas, mean, std):
    """(tensor, mask) as ``place_reference``, bit for bit, in one launch on the current stream (capturable: the images'
    pointers and sizes travel in the kernel's argument struct, nothing is uploaded and the host never waits)."""
    images = list(images)
    if not supported(images):
        raise RuntimeError("zira_place_batch does not serve these images (see canvas.supported)")
    H, W = _check(images, canvas)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std: three values each")
    lib = _lib.load()
    dev = images[0].device
    tensor = torch.empty((len(images), 3, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((len(images), H, W), dtype=torch.bool, device=dev)
    descs = (_lib.PlaceImage * len(images))()
    for d, t in zip(descs, images):
        d.data, d.h, d.w, d.stride_c, d.stride_r = t.data_ptr(), t.shape[1], t.shape[2], t.stride(0), t.stride(1)
    entry = lib.zira_place_batch_u8 if images[0].dtype == torch.uint8 else lib.zira_place_batch_f32
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        rc = entry(descs, len(images), H, W, *(float(v) for v in mean), *(float(v) for v in std), tensor.data_ptr(),
                   mask.data_ptr(), stream.cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_place_batch failed: hipError %d" % rc)
    return tensor, mask
