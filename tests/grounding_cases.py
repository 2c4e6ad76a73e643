"""Inputs of the grounding tail's tests (test_grounding_cpu.py: the op-chain twin against a numpy restatement;
test_grounding_gpu.py: the kernel against the twin), built once per case from a seed.

Shapes sit where the kernel can go wrong: Q at the wave and block edges of the scan, T at the word edges and the tail of the
float4 path, one image and three.  Values: nothing kept, everything kept, ~5 % kept with the first and the last query among
them, scores and tokens exactly AT the thresholds, eight distinct values (ties everywhere), a maximum that occurs twice, NaNs
at the first / middle / last token, exact-zero padded columns under a zero and under a negative text threshold, a different
number of valid tokens per image, and denormal probabilities (the sigmoid of a very negative logit)."""
import functools

import numpy as np
import torch

Q_EDGES = (1, 63, 64, 65, 900, 1024)
T_EDGES = (1, 31, 32, 33, 64, 255, 256)


def shapes():
    """(B, Q, T): every Q with T in {33, 256}, every T with Q in {65, 900}, B alternating between 1 and 3."""
    pairs = [(q, t) for q in Q_EDGES for t in (33, 256)] + [(q, t) for t in T_EDGES for q in (65, 900)]
    seen, out = set(), []
    for q, t in pairs:
        if (q, t) not in seen:
            seen.add((q, t))
            out.append(((1, 3)[len(out) % 2], q, t))
    return out


VALUE_SHAPES = ((3, 65, 33), (1, 900, 256), (3, 64, 32))
KINDS = ("none", "all", "sparse", "at_threshold", "ties8", "double_max", "nan", "zero_columns", "zero_columns_negative",
         "ragged_tokens", "denormal")


def _f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def make(kind, B, Q, T):
    """-> (prob [B, Q, T], boxes [B, Q, 4], box_threshold, text_threshold), CPU fp32 tensors; callers leave them unchanged."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * B + 13 * Q + T)
    rand = lambda *s: torch.rand(*s, generator=g)
    randint = lambda hi, *s: torch.randint(0, hi, s, generator=g)
    boxes = rand(B, Q, 4)
    box_thr, text_thr = 0.35, 0.25
    prob = rand(B, Q, T) * 0.3                                   # every score below 0.3
    if kind == "none":
        prob = rand(B, Q, T) * 0.9 + 0.05
        box_thr = 1.0
    elif kind == "all":
        prob = rand(B, Q, T) * 0.9 + 0.05
        box_thr = 0.0
    elif kind == "sparse":
        for b in range(B):
            rows = set(randint(Q, max(1, Q // 20)).tolist()) | {0, Q - 1}
            for q in rows:
                prob[b, q, int(randint(T, 1))] = 0.3                # a second token above the text threshold
                prob[b, q, int(randint(T, 1))] = 0.5 + 0.4 * float(rand(1))
    elif kind == "at_threshold":
        at_box, at_text = _f32(box_thr), _f32(text_thr)
        above_box = float(np.nextafter(np.float32(at_box), np.float32(1)))
        above_text = float(np.nextafter(np.float32(at_text), np.float32(1)))
        below_text = float(np.nextafter(np.float32(at_text), np.float32(0)))
        for b in range(B):
            for q in range(Q):
                prob[b, q, int(randint(T, 1))] = (at_text, above_text, below_text)[q % 3]
                if q % 4 < 2:                                       # score exactly at / one ulp above the box threshold
                    prob[b, q, int(randint(T, 1))] = at_box if q % 4 == 0 else above_box
    elif kind == "ties8":
        values = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
        # few high draws per row, so that the scores spread over several of the eight values and each is shared by many queries
        prob = values[(randint(8, B, Q, T).float() * rand(B, Q, 1)).long()]
        box_thr, text_thr = 0.45, 0.3
    elif kind == "double_max":
        prob = rand(B, Q, T) * 0.9
        if T >= 2:
            for b in range(B):
                for q in range(0, Q, 2):
                    t1, t2 = sorted(randint(T, 2).tolist())
                    prob[b, q, t1] = prob[b, q, t2] = 0.95 if q % 4 == 0 else 0.2
    elif kind == "nan":
        prob = rand(B, Q, T) * 0.6 + 0.3                          # every row would be kept
        for b in range(B):
            for q in range(Q):
                if q % 3 == 0:
                    prob[b, q, (0, T // 2, T - 1)[(q // 3) % 3]] = float("nan")
    elif kind in ("zero_columns", "zero_columns_negative"):
        prob = rand(B, Q, T) * 0.9 + 0.05
        prob[:, :, max(1, T // 3):] = 0.0                          # sigmoid(-inf) of the padded tokens
        prob[:, ::5, :] = 0.0                                      # ... and whole rows of it: score 0.0
        box_thr, text_thr = 0.0, (0.0 if kind == "zero_columns" else -0.5)
    elif kind == "ragged_tokens":
        prob = rand(B, Q, T) * 0.5
        for b in range(B):
            prob[b, :, max(1, (T * (b + 1)) // (B + 1)):] = 0.0
        box_thr, text_thr = 0.45, 0.0
    elif kind == "denormal":
        tiny = torch.tensor([0.0, 1e-45, 3e-42, 1e-39, 1.1754944e-38, 2e-38])
        prob = tiny[randint(6, B, Q, T)]
        prob[:, ::4, :] = 0.0
        box_thr, text_thr = 0.0, 0.0
    else:
        raise KeyError(kind)
    return prob.contiguous(), boxes.contiguous(), box_thr, text_thr


def all_cases():
    """(kind, B, Q, T): the shape sweep on the mixed patterns, then every value kind at the value shapes."""
    out = []
    for B, Q, T in shapes():
        out += [("sparse", B, Q, T), ("ties8", B, Q, T)]
    out += [(kind, B, Q, T) for kind in KINDS for (B, Q, T) in VALUE_SHAPES]
    return out


def case_id(c):
    return "%s-B%d-Q%d-T%d" % c
