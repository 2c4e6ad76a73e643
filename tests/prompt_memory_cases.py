"""Shared by tests/test_prompt_memory_cpu.py, tests/test_prompt_memory_gpu.py and scripts/prompt_memory_time.py: the memory
loss's case list on ``prompt_cases.Case`` (values on the 1/256 grid), the project's bar for the scalar loss, and the small model
with the text-memory switch."""
import numpy as np
import torch

import prompt_cases as cases


def small_model(dev="cpu", use_prompt_memory=True, **kw):
    """prompt_cases.small_model with ``use_prompt_memory`` in place of ``use_prompt_tuning`` (the language side branch is on)"""
    kw.setdefault("use_prompt_tuning", False)
    return cases.small_model(dev, use_prompt_memory=use_prompt_memory, **kw)


def loss_bar_holds(got, ref32, x, target):
    """The project's bar for a reduced scalar: the error of ``got`` against the float64 evaluation (of the same fp32 inputs) is at
    most twice the fp32 reference's, plus one fp32 ulp.  Returns (holds, error, bound) -- callers print before they assert."""
    exact = float((target.detach().double() - x.detach().double()).abs().mean())
    ulp = float(np.spacing(np.float32(abs(exact)))) if exact != 0.0 else float(np.finfo(np.float32).tiny)
    err, bound = abs(float(got) - exact), 2.0 * abs(float(ref32) - exact) + ulp
    return err <= bound, err, bound


def _many(B, T, n_cat, tok):
    """every image: categories c0 .. c{n-1} of ``tok`` tokens each from token 1 on; image b leaves out category b % n"""
    spans = []
    for b in range(B):
        image, t = [], 1
        for c in range(n_cat):
            if c != b % n_cat or B == 1:
                image.append(("c%d" % c, list(range(t, t + tok))))
            t += tok + 1
        assert t <= T + 1
        spans.append(image)
    return spans


def memory_cases():
    """(case, weight of the loss in front of backward).  N = B * T * D a power of two and a power-of-two weight: s = g / N is one,
    and every sum of pool-row terms is exact whatever the occurrence count; elsewhere a pool row has at most two occurrences."""
    C = cases.Case
    return [
        (C("b1_t1_d4", 1, 1, 4, [[("a", [0])]], [("a", 1)], seed=21), 1.0),
        # "b" (one row) is claimed by both images; "owl" is in the pool and in no caption, "dog" in a caption and not in the pool
        (C("b2_t7_d12", 2, 7, 12, [[("a", [1, 2]), ("b", [4])], [("b", [3]), ("dog", [1]), ("c", [5, 6])]],
           [("a", 2), ("b", 1), ("c", 2), ("owl", 2)], seed=22), 3.0),
        (C("b2_t256_d256", 2, 256, 256, _many(2, 256, 20, 11), [("c%d" % c, 11) for c in range(20)], seed=23), 0.5),
        # 4096 blocks: the fold; every pool row has 56 or 57 occurrences, exact because s = 2^-17
        (C("b64_t256_d4", 64, 256, 4, _many(64, 256, 9, 27), [("c%d" % c, 27) for c in range(9)], seed=24), 0.5),
        (C("empty_table", 2, 5, 8, [[("dog", [1])], [("dog", [2, 3])]], [("a", 1), ("owl", 2)], seed=25), 1.0),
        (C("every_row", 2, 4, 8, [[("a", [0, 1, 2, 3])], [("b", [0, 1, 2, 3])]], [("a", 4), ("b", 4)], seed=26), 1.0),
        # token 2 is in both categories' masks: the later category holds it
        (C("overlap", 1, 5, 8, [[("a", [1, 2]), ("b", [2, 3])]], [("a", 2), ("b", 2)], seed=27), 1.0),
        # D / 4 = 65 and 1024 quarter rows: a lane takes a second round (lane 0 only) and sixteen rounds
        (C("d260", 2, 3, 260, [[("a", [1])], [("b", [1]), ("a", [2])]], [("a", 1), ("b", 1)], seed=30), 3.0),
        (C("d4096", 1, 2, 4096, [[("a", [1])]], [("a", 1), ("owl", 1)], seed=31), 1.0),
        # masks of different widths (T = 9 and T = 5 padded to 9), as a batch of captions of different lengths gives them
        (C("ragged", 2, 9, 256, [[("cat", [1]), ("bear", [3, 4, 5, 6, 7])], [("cat", [1]), ("dog", [3])]],
           [("cat", 1), ("bear", 5), ("owl", 2)], widths=[9, 5], seed=32), 3.0),
        (C("declined_d6", 2, 3, 6, [[("a", [1])], [("a", [1])]], [("a", 1)], native=False, seed=28), 1.0),
        (C("declined_t257", 1, 257, 4, [[("a", [256])]], [("a", 1)], native=False, seed=29), 1.0),
    ]
