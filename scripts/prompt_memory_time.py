#!/usr/bin/env python3
"""Dev: the text-memory replay's loss (prompt.memory_loss), forward + backward through the Python calls, with the native node
(csrc/prompt_memory.hip) over a cached table and with ``memory_loss_reference`` built the naive way -- from the masks, one
boolean-mask write per image and category, the reference's loop -- in the same process.

B = 2 images that share a caption of 13 names and one of 64 names (two tokens and a separator each: 41 and 194 tokens with
[CLS] and [SEP]), D = 256, every name with a stored entry; the encoded text takes the gradient (the side branch behind it is
what trains), the entries are frozen memory.  Values on the 1/256 grid: the gradient is compared for EQUALITY and the loss is
held to the tests' bar before anything is timed.  Then warm-up and REGIONS event-timed regions of ITERS calls for each setting,
alternating; the kernel launches of one call and its synchronising calls are counted with the profiler.

Then one replay iteration end to end (``train.MemoryReplayer.run_step`` on the tests' small model with max_text_len = 256, J = 1,
64 names): the native node, the definition from the cached table (``Switches.native_prompt_memory = False``) and the
reference's loop from the masks.  Writes profiles/prompt_memory.json (or the path given as the only argument) and prints it as
one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from prompt_time import B, D, ITERS, REGIONS, counts, grid, timed  # noqa: E402
from ziragroundingdino_amd import prompt  # noqa: E402
from ziragroundingdino_amd.transformer import Switches  # noqa: E402


def step(how, x, pool, names_list, masks, table, collect=False):
    if how == "native":
        loss = prompt.memory_loss(x, table, pool)
    else:
        loss = prompt.memory_loss_reference(x, (names_list, masks), pool)
    gx, = torch.autograd.grad(loss, x)
    return (loss.detach(), gx) if collect else None


def replay_iteration(dev):
    import prompt_memory_cases as mcases
    from ziragroundingdino_amd.train import MemoryReplayer

    names = ["a%d b%d" % (i, i) for i in range(64)]
    model = mcases.small_model(dev, max_text_len=256).train()
    model.add_cls_prompt(names)
    with torch.no_grad():
        for p in model.prompt_memory_pool.values():
            p.add_(0.25)
    trainer = MemoryReplayer(model)
    tokens = int(model.encode_text([".".join(names) + "."], dev)[0]["encoded_text"].shape[1])
    pool = dict(model.prompt_memory_pool.items())
    table_loss = model._prompt_memory_loss

    def loop_loss(encoded_text, names_list, cate_to_token_mask_list, prompt_key=None):
        return prompt.memory_loss_reference(encoded_text, (names_list, cate_to_token_mask_list), pool)

    def run(how):
        Switches.native_prompt_memory = how == "native"
        model._prompt_memory_loss = loop_loss if how == "reference_loop" else table_loss
        try:
            trainer.run_step()
        finally:
            Switches.native_prompt_memory = True
            model._prompt_memory_loss = table_loss

    fns = {k: (lambda k=k: run(k)) for k in ("reference_loop", "reference_table", "native")}
    res = {"names": 64, "tokens": tokens, "J": 1, "what": "MemoryReplayer.run_step: replay_memory (frozen BERT states kept, "
           "feat_map + side branch + loss), backward, clip + AdamW on the flat bucket"}
    for k, v in timed(fns).items():
        res[k] = v
        res[k]["launches"], res[k]["synchronising_calls"] = counts(fns[k])
    return res


def main():
    import prompt_memory_cases as mcases

    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "regions": REGIONS, "calls_per_region": ITERS, "B": B, "D": D,
           "what": "forward + backward of one memory loss, the encoded text with a gradient, the entries frozen; native = "
                   "prompt.memory_loss over a cached table; reference = prompt.memory_loss_reference from the masks (one "
                   "boolean-mask index_put per image and category, then L1Loss)",
           "not_measured": "the in-step cost of a training step with use_prompt_memory on, and any AP effect"}
    for n_names in (13, 64):
        T = 3 * n_names + 2                                           # [CLS] a a . b b . ... [SEP]
        names = ["c%d" % i for i in range(n_names)]
        mask = torch.zeros(n_names, T, dtype=torch.bool)
        for c in range(n_names):
            mask[c, [1 + 3 * c, 2 + 3 * c]] = True
        names_list, masks = [names] * B, [mask.to(dev) for _ in range(B)]
        x = grid((B, T, D), gen).to(dev).requires_grad_(True)
        pool = {prompt.pool_key(n): grid((2, D), gen).to(dev) for n in names}
        keys = list(pool)
        table = prompt.build_table(names_list, masks, keys, [2] * n_names, T)
        ref = step("reference", x, pool, names_list, masks, table, collect=True)
        nat = step("native", x, pool, names_list, masks, table, collect=True)
        assert torch.equal(ref[1], nat[1]), "native gradient != reference"
        target = prompt.substitute_reference(x.detach(), table, pool)
        ok, err, bound = mcases.loss_bar_holds(nat[0], ref[0], x.detach(), target)
        assert ok and float(nat[0]) > 0, "native loss misses the bar: error %.3g, bound %.3g" % (err, bound)
        fns = {k: (lambda k=k: step(k, x, pool, names_list, masks, table)) for k in ("reference", "native")}
        res = {"names": n_names, "tokens": T, "pool_rows": 2 * n_names, "gradient_equal": True, "loss_within_bar": True,
               "loss_error": err, "loss_bound": bound}
        for k, v in timed(fns).items():
            res[k] = v
            res[k]["launches"], res[k]["synchronising_calls"] = counts(fns[k])
        out["names_%d" % n_names] = res
    out["replay_iteration"] = replay_iteration(dev)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prompt_memory.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
