"""Shared by tests/test_prompt_cpu.py, tests/test_prompt_gpu.py, scripts/prompt_time.py and the fixture's generator: the
substitution's case list -- the smallest shapes at which the kernels can still go wrong --, the small model with the
prompt-tuning switch, and the grid-valued text encoder stand-in of tests/golden/mod_prompt_tuning.pt.

Every value of a case sits on a binary grid (multiples of 1/256, bounded by 4), so every fp32 sum of a few of them is exact in
any order: the tests ask for bit equality between the kernels, the op chain and the loop on any machine."""
import torch
from torch import nn

from ziragroundingdino_amd import backbone as zb
from ziragroundingdino_amd import bert as zbert
from ziragroundingdino_amd.config import zira_swint_config
from ziragroundingdino_amd.criterion import build_criterion
from ziragroundingdino_amd.groundingdino import GroundingDINO
from ziragroundingdino_amd.transformer import build_transformer

# the fixture's classes and captions (gen_prompt_tuning_golden.py): one- and multi-token names, a class in both captions, a
# class in the pool but in no caption ("sea otter"), a class in a caption but not in the pool ("walrus")
GOLDEN_CLASSES = ["cat", "polar bear cub", "sea otter", "red fox"]
# (both tokenise to 10 tokens: in a shorter caption the [SEP] in front of the padding counts as a separator, the mask generator
# returns one mask more than there are names, and the reference's loop fails on it with an IndexError)
GOLDEN_CAPTIONS = ["cat.polar bear cub.walrus.", "red fox.cat.gray seal."]
BERT_HIDDEN = 64


def grid(shape, gen, bound=2.0, quantum=256):
    """seeded values on the grid of 1 / quantum inside [-bound, bound]"""
    return torch.round(torch.randn(*shape, generator=gen).clamp(-bound, bound) * quantum) / quantum


class GridBert(nn.Module):
    """Stand-in for the text encoder whose output sits on a binary grid: ``last_hidden_state[b, t] = table[input_ids[b, t] %
    rows]`` with table values multiples of 1/4 in [-1, 1].  No real text encoder's output can be compared bit for bit across
    machines; a lookup's can.  (``config.hidden_size`` is all the model's constructor reads.)"""

    def __init__(self, hidden=BERT_HIDDEN, rows=97, seed=11):
        super().__init__()
        self.config = zbert.BertConfig(hidden_size=hidden, num_hidden_layers=1, num_attention_heads=1, intermediate_size=hidden)
        table = torch.round(torch.randn(rows, hidden, generator=torch.Generator().manual_seed(seed)).clamp(-1, 1) * 4) / 4
        self.register_buffer("table", table)

    def forward(self, input_ids=None, **kw):
        return {"last_hidden_state": self.table[input_ids % self.table.shape[0]]}


def small_model(dev="cpu", use_prompt_tuning=True, **kw):
    """tests/test_model_gpu.py's small model (the same seed, sizes and flags) with ``use_prompt_tuning``."""
    torch.manual_seed(0)
    args = zira_swint_config(num_queries=50, enc_layers=2, dec_layers=2, dim_feedforward=128, fusion_droppath=0.0, max_text_len=32)
    swin = zb.SwinTransformer(embed_dim=24, depths=(1, 1, 2, 1), num_heads=(1, 2, 4, 8), window_size=7, drop_path_rate=0.0,
                              out_indices=(1, 2, 3))
    bb = zb.Joiner(swin, zb.PositionEmbeddingSineHW(128, 20, 20, normalize=True))
    bb.num_channels = swin.num_features[1:]
    tiny_bert = zbert.BertModel(zbert.BertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                                                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    flags = dict(num_queries=50, aux_loss=True, iter_update=True, query_dim=4, num_feature_levels=4, nheads=8,
                 two_stage_type="standard", two_stage_bbox_embed_share=False, two_stage_class_embed_share=False, max_text_len=32,
                 freeze_all=True, use_cet=True, use_project_adapter=True, select_box_nums_for_evaluation=20)
    flags.update(kw)
    model = GroundingDINO(bb, build_transformer(args), criterion=build_criterion(args), device=dev, bert=tiny_bert,
                          use_prompt_tuning=use_prompt_tuning, **flags)
    return model.to(dev)


def batch(names_per_image, height=64, width=96, seed=1, device="cpu", boxes_per_image=2):
    """train.synthetic_batch with captions in the reference's form, ``"a.b."``: the names between the separators are the
    category names the pool is keyed by"""
    from ziragroundingdino_amd.train import synthetic_batch

    data = []
    for i, names in enumerate(names_per_image):
        item = synthetic_batch(1, height, width, n_categories=len(names), boxes_per_image=boxes_per_image, seed=seed + i,
                               device=device)[0]
        item["captions"] = ".".join(names) + "."
        data.append(item)
    return data


def pred_logits(model, data):
    """eval-mode category logits [B, Q, max_text_len] of ``data``, through the model's own forward pieces"""
    from ziragroundingdino_amd.utils import nested_tensor_from_tensor_list

    with torch.no_grad():
        samples = nested_tensor_from_tensor_list(model.preprocess_image(data))
        captions, names_list = model._captions(data)
        text_dict, cate_list, loss = model.encode_text(captions, samples.device, names_list=names_list)
        features, poss = model.run_backbone(samples)
        return model.forward_features(features, poss, samples.mask, text_dict, cate_list, loss)["pred_logits"]


class Case:
    """x [B, T, D]; per image the names and token spans of its categories (``widths[b]``: the width of image b's masks);
    ``pool``: key -> [rows, D]; ``native``: inside the header's limits"""

    def __init__(self, name, B, T, D, spans, pool_rows, widths=None, native=True, seed=0):
        self.name, self.B, self.T, self.D, self.native = name, B, T, D, native
        gen = torch.Generator().manual_seed(100 + seed)
        self.x = grid((B, T, D), gen)
        self.grad = grid((B, T, D), gen)
        self.x2, self.grad2 = grid((B, T, D), gen), grid((B, T, D), gen)      # second values, for graph replays
        self.names_list = [[n for n, _ in image] for image in spans]
        self.spans = spans
        self.widths = widths or [T] * B
        self.pool = {"-%s-" % n: grid((r, D), gen) for n, r in pool_rows}
        self.pool2 = {k: grid(tuple(v.shape), gen) for k, v in self.pool.items()}

    def masks(self, device="cpu"):
        out = []
        for image, w in zip(self.spans, self.widths):
            m = torch.zeros(len(image), w, dtype=torch.bool)
            for c, (_, tokens) in enumerate(image):
                m[c, list(tokens)] = True
            out.append(m.to(device))
        return out

    def brute_force(self):
        """(b, t) -> (key, row) by walking images, categories and tokens as the reference's loop does; later writes win"""
        where = {}
        for b, image in enumerate(self.spans):
            for name, tokens in image:
                if "-%s-" % name in self.pool:
                    for i, t in enumerate(sorted(tokens)):
                        where[(b, t)] = ("-%s-" % name, i)
        return where


def cases():
    return [
        Case("one_token", 1, 1, 4, [[("a", [0])]], [("a", 1)], seed=1),
        # T = 9 and T = 5 padded to 9: [CLS] cat . polar bear cub x y [SEP] | [CLS] cat . dog [SEP]; "owl" is in the pool and in
        # no caption, "dog" in a caption and not in the pool; special tokens (0, 2, 8 | 0, 2, 4) and padding (5..8) stay
        Case("ragged", 2, 9, 256, [[("cat", [1]), ("bear", [3, 4, 5, 6, 7])], [("cat", [1]), ("dog", [3])]],
             [("cat", 1), ("bear", 5), ("owl", 2)], widths=[9, 5], seed=2),
        Case("three_images", 3, 4, 8, [[("cat", [1, 2])]] * 3, [("cat", 2)], seed=3),
        Case("last_token", 1, 256, 8, [[("a", [1]), ("z", [253, 254, 255])]], [("a", 1), ("z", 3)], seed=4),
        Case("d260", 2, 3, 260, [[("a", [1])], [("b", [1]), ("a", [2])]], [("a", 1), ("b", 1)], seed=5),
        # token 2 is in both categories' masks: the later category holds it
        Case("overlap", 1, 5, 8, [[("a", [1, 2]), ("b", [2, 3])]], [("a", 2), ("b", 2)], seed=6),
        Case("declined_d6", 2, 3, 6, [[("a", [1])], [("a", [1])]], [("a", 1)], native=False, seed=7),
        Case("declined_t257", 1, 257, 4, [[("a", [256])]], [("a", 1)], native=False, seed=8),
    ]
