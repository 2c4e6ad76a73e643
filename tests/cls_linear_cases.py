"""Shared by tests/test_cls_linear_cpu.py and tests/test_cls_linear_gpu.py: the small model with the linear-probing switch, and
the head's inputs -- text, token masks and category masks -- for a list of images."""
import torch

from ziragroundingdino_amd import backbone as zb
from ziragroundingdino_amd import bert as zbert
from ziragroundingdino_amd.config import zira_swint_config
from ziragroundingdino_amd.criterion import build_criterion
from ziragroundingdino_amd.groundingdino import GroundingDINO
from ziragroundingdino_amd.transformer import build_transformer


def small_model(dev="cpu", use_cls_linear=True, **kw):
    """tests/test_model_gpu.py's small model (the same seed, sizes and flags) with ``use_cls_linear``."""
    torch.manual_seed(0)
    args = zira_swint_config(num_queries=50, enc_layers=2, dec_layers=2, dim_feedforward=128, fusion_droppath=0.0, max_text_len=32,
                             use_cls_linear=use_cls_linear)
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
                          use_cls_linear=use_cls_linear, **flags)
    return model.to(dev)


def category_masks(spans_per_image, n_tok, dev):
    """[n_cat, n_tok[b]] bool per image from lists of token index lists"""
    masks = []
    for spans, nt in zip(spans_per_image, n_tok):
        m = torch.zeros(len(spans), nt, dtype=torch.bool)
        for c, toks in enumerate(spans):
            m[c, list(toks)] = True
        masks.append(m.to(dev))
    return masks


def text_dict(text, n_valid):
    """encoded_text [B, T, D] and its token mask: the first ``n_valid[b]`` tokens of image b are real"""
    mask = torch.zeros(text.shape[:2], dtype=torch.bool, device=text.device)
    for b, n in enumerate(n_valid):
        mask[b, :n] = True
    return {"encoded_text": text, "text_token_mask": mask}
