#!/usr/bin/env python3
"""Step time of PADDED minibatches, in the style of ab_step.py: the bench model (zira_swint_config, frozen, graph replay) and
its replayed training step, four rotating minibatches, 8 warm-up steps, then two timed runs of 20 steps.

    python scripts/padded_step.py VARIANT [--out FILE]

VARIANT  a: two 800 x 1333 images (no padding: the benchmarked step)
         b: 800 x 1333 beside 640 x 1066 (padding masks on every level), encoder attention as the fused node
            (DeformableTransformerEncoderLayer.native_padded = True, the default)
         c: the same batch with native_padded = False (the module composition of the padded layers)

Prints one JSON line (ms per step of both timed runs, and how often the fused encoder attention node ran with and without a
mask while the steps were traced and captured); ``--out`` appends it to FILE.  Run the variants alternately in ONE GPU call,
each in its own process under its own time limit: processes on one box differ by up to 0.5 ms."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ziragroundingdino_amd import encoder_layer  # noqa: E402
from ziragroundingdino_amd import transformer as zt  # noqa: E402
from ziragroundingdino_amd.config import zira_swint_config  # noqa: E402
from ziragroundingdino_amd.groundingdino import build_model  # noqa: E402
from ziragroundingdino_amd.train import ZiraTrainer, synthetic_batch  # noqa: E402

variant = sys.argv[1] if len(sys.argv) > 1 else "b"
if variant not in ("a", "b", "c"):
    raise SystemExit("variant is a, b or c")
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
zt.DeformableTransformerEncoderLayer.native_padded = variant != "c"

calls = {"padded": 0, "unpadded": 0}
_orig = encoder_layer.attention_sublayer


def _counted(*a, **k):
    calls["padded" if k.get("key_padding_mask") is not None else "unpadded"] += 1
    return _orig(*a, **k)


encoder_layer.attention_sublayer = _counted

dev = torch.device("cuda")
torch.manual_seed(0)
model = build_model(zira_swint_config(device="cuda")).to(dev).train()
trainer = ZiraTrainer(model)


def minibatch(i):
    if variant == "a":
        return synthetic_batch(2, 800, 1333, n_categories=15, seed=i, device=dev)
    return [synthetic_batch(1, 800, 1333, n_categories=15, seed=i, device=dev)[0],
            synthetic_batch(1, 640, 1066, n_categories=15, seed=100 + i, device=dev)[0]]


batches = [minibatch(i) for i in range(4)]
for i in range(8):
    trainer.run_step(batches[i % 4], next_data=batches[(i + 1) % 4])
torch.cuda.synchronize()
ts = []
for rep in range(2):
    t0 = time.perf_counter()
    for i in range(20):
        trainer.run_step(batches[i % 4], next_data=batches[(i + 1) % 4])
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) / 20 * 1e3)
line = json.dumps({"variant": variant, "images": "800x1333 + 800x1333" if variant == "a" else "800x1333 + 640x1066",
                   "native_padded": variant != "c", "ms_per_step": [round(t, 3) for t in ts],
                   "encoder_node_calls": dict(calls), "encoder_layers": len(model.transformer.encoder.layers)})
print(line, flush=True)
if out_path:
    with open(out_path, "a") as f:
        f.write(line + "\n")
