"""The phrase-grounding cases: the smallest set of shapes where the kernel can go wrong (a query count around the wave, the
eight-query step and the sorting network's sizes; a token count around the mask word and the 16-byte row; every limit once),
each with the inputs that decide it: probabilities quantised to a few levels (ties decide the order, -0.0 among them), a NaN
token inside and outside a phrase's mask, mask bits at and above T, a phrase with no bits, a phrase with ``gt_count == 0``, a
zero-area GT box, boxes that leave the frame.  Every case is matched with ``merged`` off and on.  The expected outputs come from
phrase_oracle, once per (case, merged)."""
import functools

import numpy as np
import torch

import phrase_oracle as oracle

OUTPUTS = ("top_query", "top_score", "top_iou", "first_hit", "valid")
THRS_1 = (0.5,)
THRS_10 = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)

#        name            B  Q     T    P   G   k_max thresholds
SHAPES = (("q1", 1, 1, 1, 1, 1, 10, THRS_1),                     # k_max > Q, one token, one thread's worth of everything
          ("q63_t31", 2, 63, 31, 3, 5, 10, THRS_10),
          ("q64_t32", 2, 64, 32, 3, 1, 1, THRS_1),
          ("q65_t33", 2, 65, 33, 3, 5, 32, THRS_10),
          ("q257_t195", 2, 257, 195, 3, 64, 10, THRS_1),
          ("q900_t256", 2, 900, 256, 32, 5, 10, THRS_10),        # the model's own shape
          ("q1024_t256", 1, 1024, 256, 3, 64, 32, THRS_1),       # every limit but P
          ("q20_k32", 1, 20, 64, 1, 5, 32, THRS_10))             # k_max > Q with more than one candidate


def names():
    return [s[0] for s in SHAPES]


def _word(tokens, W):
    words = np.zeros(W, np.uint32)
    for t in tokens:
        words[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return words


@functools.lru_cache(maxsize=None)
def get(name):
    i, (_, B, Q, T, P, G, K, thrs) = next((i, s) for i, s in enumerate(SHAPES) if s[0] == name)
    rng = np.random.default_rng(100 + i)
    W = (T + 31) // 32
    levels = np.array([0.0, -0.0, 0.125, 0.25, 0.5, 0.5, 0.75, 0.875], np.float32)
    prob = levels[rng.integers(0, len(levels), (B, Q, T))]
    boxes = np.concatenate([rng.uniform(-0.05, 1.05, (B, Q, 2)), rng.uniform(0.05, 0.6, (B, Q, 2))], -1).astype(np.float32)
    sizes = np.array([[480.0, 640.0], [333.0, 500.0]], np.float32)[:B]
    bits = np.zeros((B, P, W), np.uint32)
    for b in range(B):
        for p in range(P):
            n = T if p == 1 and (Q <= 300 or Q == 1024) else int(rng.integers(1, 5))      # every token / a few, as phrases are
            bits[b, p] = _word(rng.choice(T, min(n, T), replace=False).tolist(), W)
    if T % 32:
        bits[:, :, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(T % 32)          # bits at and above T: never looked at
    # ground truth: boxes of the phrase's better queries, moved a little, in pixels; the rest anywhere
    gt = np.zeros((B, P, G, 4), np.float32)
    count = np.zeros((B, P), np.int32)
    for b in range(B):
        h, w = sizes[b]
        for p in range(P):
            count[b, p] = rng.integers(1, G + 1)
            for g in range(G):
                cx, cy, bw, bh = boxes[b, rng.integers(0, Q)] * (1 + rng.uniform(-0.15, 0.15, 4))
                gt[b, p, g] = (max((cx - bw / 2) * w, 0), max((cy - bh / 2) * h, 0), min((cx + bw / 2) * w, w), min((cy + bh / 2) * h, h))
    gt[0, 0, 0, 2] = gt[0, 0, 0, 0]                                            # a zero-area GT box
    if G > 1:
        count[0, 0] = G
        gt[0, 0, 1] = oracle.pixel_box(boxes[0, 0], sizes[0, 0], sizes[0, 1])  # ... beside the exact box of query 0
    if Q > 2:
        tokens = oracle.phrase_tokens(bits[0, 0].view(np.int32), T)
        prob[0, 1, tokens[0]] = np.nan                                         # a NaN inside phrase 0's mask: query 1 ranks first
        outside = [t for t in range(T) if t not in tokens]
        if outside:
            prob[0, 2, outside[0]] = np.nan                                    # ... and outside it: query 2 is as it was
    if P >= 3:
        bits[0, 2] = 0                                                         # a phrase with no bits ...
        if T % 32:
            bits[0, 2, -1] = np.uint32(0xFFFFFFFF) << np.uint32(T % 32)        # ... below T
        count[B - 1, 0] = 0                                                    # a phrase without ground truth
        count[B - 1, 2] = -3                                                   # (clamped)
    return dict(name=name, prob=prob, boxes=boxes, sizes=sizes, phrase_bits=bits.view(np.int32), gt_boxes=gt, gt_count=count,
                k_max=K, iou_thrs=thrs)


INPUTS = ("prob", "boxes", "sizes", "phrase_bits", "gt_boxes", "gt_count")


def tensors(case, device="cpu"):
    return tuple(torch.from_numpy(case[k]).to(device) for k in INPUTS)


@functools.lru_cache(maxsize=None)
def expected(name, merged):
    case = get(name)
    return oracle.match(*(case[k] for k in INPUTS), case["k_max"], case["iou_thrs"], merged)


def as_numpy(match):
    return {k: getattr(match, k).cpu().numpy() for k in OUTPUTS}


def assert_equal(got, want, what):
    """Bit for bit: the floats are compared as their integer patterns (a NaN score is one pattern)."""
    for k in OUTPUTS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype.kind == "f":
            g, w = g.view("i%d" % g.dtype.itemsize), w.view("i%d" % w.dtype.itemsize)
        assert np.array_equal(g, w), "%s: %s differs at %s" % (what, k, np.argwhere(g != w)[:5].tolist())
