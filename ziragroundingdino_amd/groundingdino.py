"""ZiRa GroundingDINO model -- drop-in for the reference's
``groundingdino/models/GroundingDINO/groundingdino_dual_zero_rep_branch.py`` (class
``GroundingDINO`` :137-745, builder :748-827, registry name ``dualzerorepbranchgroundingdino``).

Same surface: ``model(batched_inputs)`` with ``[{"image": uint8/float [3,H,W], "captions":
"cat . dog .", "instances": Instances}]`` returns the weighted loss dict in training mode
(``loss_class/_bbox/_giou`` + ``_0.._4`` + ``_enc``, ``loss_conv_adapter``,
``loss_linear_adapter``; with ``use_adapter`` and ``use_self_kd`` both on also ``loss_adapter``, the transformer's adapter
loss times ``loss_adapter_weight`` -- a stated departure: the reference's dual-branch class receives that loss and drops it
(:532), its sibling classes add it (groundingdino_repconv.py:673-679), and a baseline whose switch does nothing is no
baseline) and ``[{"instances": Instances}]`` in eval mode; the hooks
``before_train`` / ``after_train`` / ``add_cls_prompt`` / ``load_state_dict`` and the
parameter names (``input_proj_conv_adapter.N.*``, ``rep_linear_adapter.*``, ``feat_map``,
``input_proj``, ``bbox_embed``, ``transformer.*``, ``backbone.0.*``, ``bert.*``) are the
reference's, so its checkpoints and its training driver work unchanged.

What runs where: both side branches go through the fused RSB epilogue kernels (rsb.py), all
12 deformable-attention calls through the gfx950 MSDA kernels (ms_deform_attn.py); the frozen
backbone and text encoder are stock PyTorch-ROCm and are evaluated without building an
autograd graph (nothing upstream of the side branches needs gradients).
"""
import copy
import os
import random
from typing import List

import torch
import torch.nn.functional as F
from torch import nn

from .backbone import build_backbone
from .bert import BertConfig, BertModel, SimpleTokenizer
from . import canvas
from .box_ops import box_cxcywh_to_xyxy, box_xyxy_to_cxcywh
from .criterion import build_criterion
from .dense import conv_module_as_gemm
from .graphs import GraphedNoGrad, GraphedTransformer
from .rsb import RepZeroConv2d, RepZeroLinear, RepZeroLoRA
from .structures import Boxes, ImageList, Instances
from .text_masks import generate_masks_with_special_tokens_and_transfer_map
from .transformer import build_transformer
from .utils import (MLP, ContrastiveEmbed, ContrastiveEmbedwithLinear, NestedTensor, box_head, inverse_sigmoid,
                    nested_tensor_from_tensor_list, recover_to_cls_logits)


class _Registry:
    """name -> builder, as groundingdino/models/registry.py ``MODULE_BUILD_FUNCS``."""

    def __init__(self):
        self._funcs = {}

    def registe_with_name(self, module_name=None, force=False):
        def deco(fn):
            name = module_name or fn.__name__
            if name in self._funcs and not force:
                raise KeyError("%s is already registered" % name)
            self._funcs[name] = fn
            return fn
        return deco

    def get(self, name):
        return self._funcs[name]

    def __contains__(self, name):
        return name in self._funcs


MODULE_BUILD_FUNCS = _Registry()


class GroundingDINO(nn.Module):
    # postprocess: class-aware NMS (nms.py) of the detections at this IoU; None = none, what the reference's evaluation does
    nms_threshold_for_evaluation = None
    # eval-mode forward: a category list that tokenises longer than max_text_len runs in chunks that fit and the chunks'
    # detections are merged on the device (vocab.py).  None = one caption, cut at max_text_len as ever; "auto" = split by the
    # token budget; an int = that, and at most so many names per chunk
    category_chunk_size = None

    def __init__(self, backbone, transformer, num_queries, aux_loss=False, iter_update=False,
                 query_dim=2, num_feature_levels=1, nheads=8, two_stage_type="no",
                 dec_pred_bbox_embed_share=True, two_stage_class_embed_share=True,
                 two_stage_bbox_embed_share=True, num_patterns=0, dn_number=100,
                 dn_box_noise_scale=0.4, dn_label_noise_ratio=0.5, dn_labelbook_size=100,
                 text_encoder_type="bert-base-uncased", sub_sentence_present=True, max_text_len=256,
                 criterion=None, pixel_mean: List[float] = [123.675, 116.280, 103.530],
                 pixel_std: List[float] = [123.675, 116.280, 103.530], device="cuda",
                 select_box_nums_for_evaluation=200, freeze_all=False, loss_adapter_weight=0.1,
                 use_cet=False, use_prompt_memory=False, num_select_prompt=200,
                 use_zero_inter_loss=True, use_add_names=False, use_bert_tuning=False,
                 use_cls_linear=False, use_prompt_tuning=False, use_prompt_memory_output=True,
                 use_project_tuning=False, use_project_adapter=True,
                 use_zero_inter_loss_for_conv=True, use_learned_names=False,
                 bert=None, tokenizer=None, side_branch="rep", use_adapter=False, use_self_kd=False,
                 text_branch="rep", cet_type="Adapter", cet_middle_dim=1024, zero_loss_type="L1", lora_down_dim=None,
                 **_unused):
        super().__init__()
        assert query_dim == 4 and iter_update, "GroundingDINO uses 4-d queries with iterative update"
        assert two_stage_type in ["no", "standard"]
        self.num_queries = num_queries
        self.transformer = transformer
        self.hidden_dim = hidden_dim = transformer.d_model
        self.num_feature_levels = num_feature_levels
        self.nheads = nheads
        self.max_text_len = max_text_len
        self.sub_sentence_present = sub_sentence_present
        self.query_dim = query_dim
        self.num_patterns = num_patterns
        self.dn_number, self.dn_box_noise_scale = dn_number, dn_box_noise_scale
        self.dn_label_noise_ratio, self.dn_labelbook_size = dn_label_noise_ratio, dn_labelbook_size

        # text encoder (frozen); tokenizer / pretrained weights can be injected by the caller
        self.tokenizer = tokenizer if tokenizer is not None else SimpleTokenizer()
        self.bert = bert if bert is not None else BertModel(BertConfig())
        self.bert.pooler.dense.weight.requires_grad_(False)
        self.bert.pooler.dense.bias.requires_grad_(False)
        self.feat_map = nn.Linear(self.bert.config.hidden_size, hidden_dim, bias=True)
        nn.init.constant_(self.feat_map.bias.data, 0)
        nn.init.xavier_uniform_(self.feat_map.weight.data)

        self.learned_classes = []
        self.use_cet = use_cet
        self.use_prompt_memory = use_prompt_memory
        self.use_zero_inter_loss = use_zero_inter_loss
        self.prompt_memory_pool = nn.ParameterDict()
        self.num_select_prompt = num_select_prompt
        self.use_prompt_tuning = use_prompt_tuning
        self.use_learned_names = use_learned_names
        self.use_prompt_memory_output = use_prompt_memory_output
        # "rep": the ZiRa model (groundingdino_dual_zero_rep_branch.py); "multilayer": its multilayer-branch
        # ablation (groundingdino_dual_zero_rep_multilayer_branch.py, rsb_multilayer.py)
        assert side_branch in ("rep", "multilayer")
        self.side_branch = side_branch
        # "rep": ZiRa's RepZeroLinear beside feat_map; "cet": the sibling class's trained text adapter in its place
        # (groundingdino_dt.py:182-215, cet.py) -- ``use_cet`` then builds ``cet_adapter``, which nothing merges; "lora": the
        # low-rank form of ZiRa's branch under the same name (adapter.py:227-259, rsb.RepZeroLoRA), merged like the dense one
        assert text_branch in ("rep", "cet", "lora")
        if text_branch == "lora" and side_branch != "rep":
            raise ValueError('text_branch="lora" goes with side_branch="rep": the multilayer ablation has a language branch of its own')
        if text_branch == "cet":
            from . import cet

            if side_branch != "rep":
                raise ValueError('text_branch="cet" goes with side_branch="rep": the multilayer ablation has a language branch of its own')
            if zero_loss_type not in cet.LOSS_CODES:
                raise NotImplementedError("zero_loss_type %r: one of L1, L2, Smooth_L1" % (zero_loss_type,))
            if use_prompt_memory and zero_loss_type != "L1":
                raise NotImplementedError("use_prompt_memory with zero_loss_type %r: the memory loss (prompt.memory_loss) is the L1 "
                                          "mean only" % (zero_loss_type,))
            self.cet_type, self.zero_loss_type = cet_type, zero_loss_type
        self.text_branch = text_branch
        if side_branch == "multilayer":  # unconditional language branch, its own name (reference :322-323)
            from . import rsb_multilayer

            self.rep_language_adapter = rsb_multilayer.RepZeroLinear(self.bert.config.hidden_size, hidden_dim)
            conv_branch = rsb_multilayer.RepZeroConv2dGN
        else:
            conv_branch = RepZeroConv2d
            if use_cet and text_branch == "cet":
                self.cet_adapter = cet.build_cet_adapter(cet_type, self.bert.config.hidden_size, cet_middle_dim, hidden_dim)
            elif use_cet and text_branch == "lora":
                self.rep_linear_adapter = RepZeroLoRA(self.bert.config.hidden_size, hidden_dim, down_dim=lora_down_dim)
            elif use_cet:  # RSB #1: language side branch beside feat_map
                self.rep_linear_adapter = RepZeroLinear(self.bert.config.hidden_size, hidden_dim)
        self.specical_tokens = self.tokenizer.convert_tokens_to_ids(["[CLS]", "[SEP]", ".", "?"])

        # input projections (frozen) and RSB #2: one zero-initialised conv branch beside each
        chans = list(backbone.num_channels)
        proj, adapters = [], []
        in_channels = chans[-1]
        if num_feature_levels > 1:
            for c in chans:
                proj.append(nn.Sequential(nn.Conv2d(c, hidden_dim, kernel_size=1), nn.GroupNorm(32, hidden_dim)))
                adapters.append(conv_branch(c, hidden_dim, kernel_size=1))
            for _ in range(num_feature_levels - len(chans)):
                proj.append(nn.Sequential(nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1),
                                          nn.GroupNorm(32, hidden_dim)))
                adapters.append(conv_branch(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1))
                in_channels = hidden_dim
        else:
            assert two_stage_type == "no"
            proj.append(nn.Sequential(nn.Conv2d(chans[-1], hidden_dim, kernel_size=1), nn.GroupNorm(32, hidden_dim)))
            adapters.append(conv_branch(chans[-1], hidden_dim, kernel_size=1))
        self.input_proj = nn.ModuleList(proj)
        self.use_project_adapter = use_project_adapter
        self.use_zero_inter_loss_for_conv = use_zero_inter_loss_for_conv
        if use_project_adapter:
            self.input_proj_conv_adapter = nn.ModuleList(adapters)

        self.backbone = backbone
        self.aux_loss = aux_loss
        self.box_pred_damping = None
        self.iter_update = iter_update

        # prediction heads, shared across decoder layers
        self.dec_pred_bbox_embed_share = dec_pred_bbox_embed_share
        if use_cls_linear:   # linear probing: the classifier gets a trained linear in front of the text product (reference :317-321)
            _class_embed = ContrastiveEmbedwithLinear(max_text_len=max_text_len, hidden_dim=hidden_dim)
        else:
            _class_embed = ContrastiveEmbed(max_text_len=max_text_len)
        _bbox_embed = MLP(hidden_dim, hidden_dim, 4, 3)
        nn.init.constant_(_bbox_embed.layers[-1].weight.data, 0)
        nn.init.constant_(_bbox_embed.layers[-1].bias.data, 0)
        n_dec = transformer.num_decoder_layers
        boxes = [_bbox_embed if dec_pred_bbox_embed_share else copy.deepcopy(_bbox_embed) for _ in range(n_dec)]
        self.bbox_embed = nn.ModuleList(boxes)
        self.class_embed = nn.ModuleList([_class_embed for _ in range(n_dec)])
        self.transformer.decoder.bbox_embed = self.bbox_embed
        self.transformer.decoder.class_embed = self.class_embed
        self.two_stage_type = two_stage_type
        if two_stage_type != "no":
            if two_stage_bbox_embed_share:
                assert dec_pred_bbox_embed_share
                self.transformer.enc_out_bbox_embed = _bbox_embed
            else:
                self.transformer.enc_out_bbox_embed = copy.deepcopy(_bbox_embed)
            if two_stage_class_embed_share:
                assert dec_pred_bbox_embed_share
                self.transformer.enc_out_class_embed = _class_embed
            else:
                self.transformer.enc_out_class_embed = copy.deepcopy(_class_embed)
            self.refpoint_embed = None

        self.criterion = criterion
        self.pixel_mean, self.pixel_std = pixel_mean, pixel_std
        self._pixel_stats = {}
        self._text_cache = {}
        self._prompt_tables = {}     # use_prompt_tuning / use_prompt_memory: the index tables per caption set (prompt.py)
        self._replay_cache = None    # replay_memory: the frozen BERT's states of the learned classes' captions
        self.device = device
        self._reset_parameters()
        self.use_add_names = use_add_names
        self.select_box_nums_for_evaluation = select_box_nums_for_evaluation
        self.loss_adapter_weight = loss_adapter_weight
        self.use_adapter, self.use_self_kd = use_adapter, use_self_kd
        self.freeze_all = freeze_all
        self.use_bert_tuning = use_bert_tuning
        self.use_cls_linear = use_cls_linear
        self.use_project_tuning = use_project_tuning
        # hipGraph replay of the frozen front end (GPU only; see graphs.py)
        self.use_frontend_graphs = True
        self._graphed_backbone = GraphedNoGrad(self._backbone_tensors, modules=(self.backbone,))
        self._graphed_bert = GraphedNoGrad(self._bert_hidden, modules=(self.bert,))
        # hipGraph replay of transformer forward + backward (training mode on the GPU with the transformer
        # frozen -- every ZiRa task; up to two input signatures, further ones run eagerly); see
        # graphs.GraphedTransformer.  On by default since round 3 (2000-step soak over rotating minibatches,
        # scripts/soak_graph.py; two ranks sharing a GPU, tests/test_model_gpu.py); False launches eagerly.
        # As with any torch.cuda.make_graphed_callables callable: ONE backward per forward (no retain_graph re-runs).
        self.use_transformer_graph = True
        self.overlap_text_and_image = True   # frozen BERT replayed on a side stream while the frozen Swin runs
        self._text_stream = None
        self._prefetch_stream = None
        self._graphed_transformer = GraphedTransformer(self.transformer)
        self._canvas_sizes = None

    # Canvas batching (canvas.py), off by default.  None: a minibatch is padded to its own maximum, as the reference does.  A list
    # of (H, W), e.g. ``canvas.DEFAULT_CANVASES``: it is padded to the smallest canvas that holds it, by one launch, so that a
    # stream of image sizes meets a handful of shapes and keeps replaying from hipGraphs; the graph caches then hold one entry per
    # canvas and drop the least recently used one instead of going eager (graphs.py ``evict_lru``).  A batch that no canvas holds
    # takes the path of None.
    @property
    def canvas_sizes(self):
        return self._canvas_sizes

    @canvas_sizes.setter
    def canvas_sizes(self, sizes):
        sizes = None if sizes is None else [(int(h), int(w)) for h, w in sizes]
        if sizes is not None and not sizes:
            raise ValueError("canvas_sizes: None or at least one (H, W)")
        self._canvas_sizes = sizes
        on = sizes is not None
        self._graphed_backbone.evict_lru = self._graphed_bert.evict_lru = self._graphed_transformer.evict_lru = on
        self._graphed_backbone.max_signatures = len(sizes) if on else 8
        self._graphed_transformer.max_signatures = len(sizes) if on else 2

    def _canvas_batch(self, batched_inputs):
        """(images, samples) of a minibatch on the canvas ``canvas.choose`` picks for its largest height and width (both known on
        the host), or (None, None) where no canvas holds it.  ``images.image_sizes`` stay the real sizes: targets and detections
        are scaled per image, and the valid ratios come from the mask."""
        raw = [x["image"].to(self.device) for x in batched_inputs]
        sizes = [(t.shape[-2], t.shape[-1]) for t in raw]
        cv = canvas.choose(max(s[0] for s in sizes), max(s[1] for s in sizes), self._canvas_sizes)
        if cv is None:
            return None, None
        if canvas.supported(raw):
            tensor, mask = canvas.place(raw, cv, self.pixel_mean, self.pixel_std)
        else:   # CPU tensors, other dtypes / layouts, more than 8 images: the op chain, padded to the canvas
            tensor, mask = canvas.place_reference(raw, cv, self.pixel_mean, self.pixel_std)
        samples = NestedTensor(tensor, mask)
        samples.no_padding = all(tuple(s) == cv for s in sizes)   # known on the host
        return ImageList(tensor, sizes), samples

    def _backbone_tensors(self, images, mask):
        """tensor-in / tensor-out view of the backbone for graph capture."""
        features, poss = self.backbone(NestedTensor(images, mask))
        return [f.tensors for f in features], [f.mask for f in features], poss

    def _bert_hidden(self, enc_in):
        return self.bert(**enc_in)["last_hidden_state"]

    def run_backbone(self, samples):
        """features (list of NestedTensor) and position encodings of the frozen backbone."""
        if self._frozen(self.backbone):
            if self.use_frontend_graphs and samples.tensors.is_cuda:
                ft, fm, poss = self._graphed_backbone(samples.tensors, samples.mask)
            else:
                with torch.no_grad():
                    ft, fm, poss = self._backbone_tensors(samples.tensors, samples.mask)
            return [NestedTensor(t, m) for t, m in zip(ft, fm)], list(poss)
        return self.backbone(samples)

    def _reset_parameters(self):
        for proj in self.input_proj:
            nn.init.xavier_uniform_(proj[0].weight, gain=1)
            nn.init.constant_(proj[0].bias, 0)

    def init_ref_points(self, use_num_queries):
        self.refpoint_embed = nn.Embedding(use_num_queries, self.query_dim)

    # ---- pieces of forward ----------------------------------------------------------------
    @staticmethod
    def _frozen(module):
        """No parameter of ``module`` requires grad.  Checked on every forward (the answer may change
        between calls), but on a remembered flat list: ``module.parameters()`` walks the module tree
        (0.7 ms for Swin / BERT), reading ``requires_grad`` of 370 tensors does not."""
        params = getattr(module, "_zira_param_list", None)
        if params is None:
            params = list(module.parameters())
            object.__setattr__(module, "_zira_param_list", params)
        return not any(p.requires_grad for p in params)

    def _loss_weights(self, name, suffixes, weight_dict, like):
        key = (name, tuple(suffixes), tuple(weight_dict[name + suf] for suf in suffixes), like.device, like.dtype)
        cache = self.__dict__.setdefault("_loss_weight_cache", {})
        w = cache.get(key)
        if w is None:
            w = cache[key] = torch.tensor(key[2], dtype=like.dtype).to(like.device)
        return w

    def _project_level(self, l, feat):
        """GroupNorm(input_proj conv + side branch); returns (src, zero-interference loss | None)."""
        from .dense import group_norm_frozen, group_norm_supported
        main = conv_module_as_gemm(self.input_proj[l][0], feat)  # GEMM library instead of MIOpen
        gn = self.input_proj[l][1]
        if not self.use_project_adapter:
            return (group_norm_frozen(main, gn) if group_norm_supported(main, gn) else gn(main)), None
        branch, zero_loss = self.input_proj_conv_adapter[l](feat)
        if self.side_branch == "multilayer":   # the branch carries its own GroupNorm (reference :575-576)
            return (group_norm_frozen(main, gn) if group_norm_supported(main, gn) else gn(main)) + branch, zero_loss
        if group_norm_supported(main, gn, branch):   # the sum is formed inside the kernel (csrc/groupnorm.hip)
            return group_norm_frozen(main, gn, branch), zero_loss
        return gn(main + branch), zero_loss

    def _encoder_inputs(self, captions, device):
        """(tokenized, masks, position_ids, cate_to_token_mask_list, enc_in) of ``captions`` on ``device``."""
        # Tokenisation, the sub-sentence masks and their upload are a pure function of the caption
        # strings, and a task trains on one category list for thousands of steps: remembered per
        # (captions, device) instead of redone every step (2.5 ms of host time, five blocking copies).
        key = (tuple(captions), str(device))
        cached = self._text_cache.get(key)
        if cached is None:
            tokenized = self.tokenizer(captions, padding="longest", return_tensors="pt").to(device)
            masks, position_ids, cate_to_token_mask_list = generate_masks_with_special_tokens_and_transfer_map(
                tokenized, self.specical_tokens, self.tokenizer)
            L = self.max_text_len
            if masks.shape[1] > L:
                masks = masks[:, :L, :L]
                position_ids = position_ids[:, :L]
                for k in ("input_ids", "attention_mask", "token_type_ids"):
                    tokenized[k] = tokenized[k][:, :L]
            if self.sub_sentence_present:
                enc_in = {k: v for k, v in tokenized.items() if k != "attention_mask"}
                enc_in["attention_mask"] = masks
                enc_in["position_ids"] = position_ids
            else:
                enc_in = tokenized
            if len(self._text_cache) >= 64:
                self._text_cache.clear()
            cached = self._text_cache[key] = (tokenized, masks, position_ids, cate_to_token_mask_list, dict(enc_in))
        return cached

    def encode_text(self, captions, device, defer=False, hidden_only=False, names_list=None, bert_hidden=None):
        # ``names_list`` (the captions' category names): with ``use_prompt_tuning`` the pool entries of these categories replace
        # their tokens (project_text), with ``use_prompt_memory`` they are the memory loss's targets in training and replace
        # their tokens in eval; None -- free text, no category list -- substitutes nothing and computes no memory loss
        # ``bert_hidden``: the text encoder's states for these captions where the caller holds them (replay_memory, frozen
        # BERT): the encoder is not run
        key = (tuple(captions), str(device))
        tokenized, masks, position_ids, cate_to_token_mask_list, enc_in = self._encoder_inputs(captions, device)
        enc_in = dict(enc_in)
        side = None
        if bert_hidden is not None:
            hidden = bert_hidden
        elif self._frozen(self.bert):
            if self.use_frontend_graphs and enc_in["input_ids"].is_cuda:
                if defer and self.overlap_text_and_image:
                    # the frozen BERT (a graph of ~300 launch-bound kernels) runs beside the frozen Swin: its replay
                    # goes to a side stream here and is joined in finish(), after the caller has queued the backbone
                    if self._text_stream is None:
                        self._text_stream = torch.cuda.Stream(device=device)
                    side = self._text_stream
                    side.wait_stream(torch.cuda.current_stream(device))
                    with torch.cuda.stream(side):
                        hidden = self._graphed_bert(enc_in)
                else:
                    hidden = self._graphed_bert(enc_in)
            else:
                with torch.no_grad():
                    hidden = self._bert_hidden(enc_in)
        else:
            hidden = self._bert_hidden(enc_in)

        def finish():
            if side is not None:
                torch.cuda.current_stream(device).wait_stream(side)
                hidden.record_stream(torch.cuda.current_stream(device))
            elif hidden_only and hidden.is_cuda:   # computed on a prefetch stream; the caller has waited for it
                hidden.record_stream(torch.cuda.current_stream(device))
            text_dict, loss_linear_adapter = self.project_text(
                hidden, tokenized["attention_mask"].bool(), position_ids, masks, names_list=names_list,
                cate_to_token_mask_list=cate_to_token_mask_list, prompt_key=key)
            return text_dict, cate_to_token_mask_list, loss_linear_adapter

        return (finish, cate_to_token_mask_list) if defer else finish()

    def project_text(self, bert_hidden, text_token_mask, position_ids, text_self_attention_masks, names_list=None,
                     cate_to_token_mask_list=None, prompt_key=None):
        """feat_map + language side branch (reference :459-476): BERT states -> text_dict.  With ``use_prompt_tuning`` and a
        category list, the pool entries then replace their categories' tokens (the sibling class's groundingdino_dt.py:521-531),
        in training and in eval, in front of the ``max_text_len`` cut.

        With ``use_cet and use_prompt_memory`` (the sibling class's text-memory replay) and a category list:

        * in training, ``text_dict["loss_prompt_memory"]`` is the L1 distance (mean) between the encoded text behind the side
          branch and its copy with the rows of every category in ``learned_classes`` overwritten by the stored entry (:509-519),
          taken in front of any substitution and of the cut; ``forward_features`` takes the key out again;
        * in eval, with ``use_prompt_memory_output`` as well, the stored rows replace the tokens of every category that has an
          entry (:521-531).  Two departures from groundingdino_dt.py: ``use_prompt_memory_output`` alone does nothing (its
          default here is True, and making it live by itself would change every existing evaluation), and the side branch keeps
          running in eval (the dual-branch class this package mirrors always runs it; after the merge it is the 1e-8
          initialisation).

        With ``text_branch="cet"`` (:499-507): ``feat_map`` first, then the CET adapter on the BERT STATES (not on the projected
        text), added to the projected text, with its zero-interference term as the second return value (cet.cet_apply).  It
        runs only when ``self.training or not self.use_prompt_memory_output``: as in the reference, an eval-mode forward under
        the default ``use_prompt_memory_output=True`` skips the adapter altogether -- the stored rows are meant to stand in for
        it -- and the encoded text is ``feat_map``'s alone (the eval substitution itself keeps this package's condition: both
        ``use_prompt_memory`` and ``use_prompt_memory_output``)."""
        L = self.max_text_len
        encoded_text = self.feat_map(bert_hidden)
        loss_linear_adapter = None
        if self.text_branch == "cet":
            if self.use_cet and (self.training or not self.use_prompt_memory_output):
                from . import cet

                encoded_text, loss_linear_adapter = cet.cet_apply(bert_hidden, encoded_text, self.cet_adapter, self.zero_loss_type,
                                                                  self.use_zero_inter_loss)
        elif self.side_branch == "multilayer":
            rep_out, loss_linear_adapter = self.rep_language_adapter(bert_hidden)
            encoded_text = rep_out + encoded_text
        elif self.use_cet:
            rep_out, loss_linear_adapter = self.rep_linear_adapter(bert_hidden)
            encoded_text = rep_out + encoded_text
        loss_prompt_memory = None
        if self.use_cet and self.use_prompt_memory and self.training and names_list is not None:
            loss_prompt_memory = self._prompt_memory_loss(encoded_text, names_list, cate_to_token_mask_list, prompt_key)
        substitutes = self.use_prompt_tuning or (self.use_prompt_memory and self.use_prompt_memory_output and not self.training)
        if substitutes and names_list is not None and len(self.prompt_memory_pool):
            encoded_text = self._substitute_prompts(encoded_text, names_list, cate_to_token_mask_list, prompt_key)
        if encoded_text.shape[1] > L:
            encoded_text, text_token_mask = encoded_text[:, :L, :], text_token_mask[:, :L]
            position_ids = position_ids[:, :L]
            text_self_attention_masks = text_self_attention_masks[:, :L, :L]
        text_dict = {"encoded_text": encoded_text, "text_token_mask": text_token_mask,
                     "position_ids": position_ids,
                     "text_self_attention_masks": text_self_attention_masks}
        if loss_prompt_memory is not None:
            text_dict["loss_prompt_memory"] = loss_prompt_memory
        return text_dict, loss_linear_adapter

    def _prompt_names(self, names_list):
        """``encode_text``'s keyword for the category list: only with ``use_prompt_tuning`` or ``use_prompt_memory`` -- without
        them the call is what it was."""
        return {"names_list": names_list} if (self.use_prompt_tuning or self.use_prompt_memory) else {}

    def _prompt_table(self, names_list, cate_to_token_mask_list, keys, T, D, prompt_key):
        """The index tables (prompt.py) of ``names_list`` against the pool entries ``keys``: built once per caption set
        (``prompt_key``: the text cache's key) and pool version -- the one host read of the masks -- and dropped when
        ``add_cls_prompt`` or ``load_state_dict`` changes the pool."""
        from . import prompt

        pool = self.prompt_memory_pool
        key = None if prompt_key is None else (prompt_key, tuple(tuple(names) for names in names_list), T, tuple(keys))
        table = self._prompt_tables.get(key) if key is not None else None
        if table is None:
            for k in keys:
                if pool[k].dim() != 2 or pool[k].shape[1] != D:
                    raise ValueError("prompt pool entry %s has shape %s, not [n_tok, %d]: it does not come from a prompt-tuning or "
                                     "prompt-memory run" % (k, tuple(pool[k].shape), D))
            table = prompt.build_table(names_list, cate_to_token_mask_list, keys, [pool[k].shape[0] for k in keys], T)
            if key is not None:
                if len(self._prompt_tables) >= 64:
                    self._prompt_tables.clear()
                self._prompt_tables[key] = table
        return table

    def _prompt_memory_loss(self, encoded_text, names_list, cate_to_token_mask_list, prompt_key=None):
        """``loss_prompt_memory`` (groundingdino_dt.py:509-519): the categories of ``names_list`` that are in ``learned_classes``
        are pulled back to their stored rows.  A learned class without an entry raises, as the reference's lookup does."""
        from . import prompt

        pool = self.prompt_memory_pool
        learned = set(self.learned_classes)
        wanted = {prompt.pool_key(n) for names in names_list for n in names if n in learned}
        missing = sorted(k for k in wanted if k not in pool)
        if missing:
            raise KeyError("use_prompt_memory: learned classes without a pool entry: %s" % ", ".join(missing))
        keys = [k for k in pool.keys() if k in wanted]
        if not keys:      # nothing learned yet (the first task): target == encoded_text
            return prompt.memory_loss_reference(encoded_text, (names_list, cate_to_token_mask_list), {})
        table = self._prompt_table(names_list, cate_to_token_mask_list, keys, encoded_text.shape[1], encoded_text.shape[-1], prompt_key)
        return prompt.memory_loss(encoded_text, table, [pool[k] for k in keys])

    def _substitute_prompts(self, encoded_text, names_list, cate_to_token_mask_list, prompt_key=None):
        """``encoded_text`` with the tokens of every category that has a pool entry replaced by the entry (prompt.py).  The index
        tables are built once per caption set (``prompt_key``: the text cache's key) and pool version -- the one host read of the
        masks -- and dropped when ``add_cls_prompt`` or ``load_state_dict`` changes the pool."""
        from . import prompt

        pool = self.prompt_memory_pool
        wanted = {prompt.pool_key(n) for names in names_list for n in names}
        keys = [k for k in pool.keys() if k in wanted]
        if not keys:
            return encoded_text
        table = self._prompt_table(names_list, cate_to_token_mask_list, keys, encoded_text.shape[1], encoded_text.shape[-1], prompt_key)
        return prompt.substitute(encoded_text, table, [pool[k] for k in keys])

    def _captions(self, batched_inputs):
        captions = [x["captions"] for x in batched_inputs]
        names_list = [x["captions"][:-1].split(".") for x in batched_inputs]
        if (self.use_add_names and not self.training) or (self.use_learned_names and self.training):
            extra = [c for c in self.learned_classes if c not in names_list[0]]
            if self.training and len(extra) >= self.num_select_prompt:
                extra = random.sample(extra, self.num_select_prompt)
            for i, (caption, names) in enumerate(zip(captions, names_list)):
                names_list[i] = names + extra
                captions[i] = caption + ".".join(extra)
                if not captions[i].endswith("."):
                    captions[i] += "."
        return captions, names_list

    def can_prefetch_frontend(self):
        return (self.training and self.use_frontend_graphs and self._frozen(self.backbone) and self._frozen(self.bert)
                and next(self.parameters()).is_cuda)

    def prefetch_frontend(self, batched_inputs):
        """Queue the FROZEN front end (image normalisation, Swin, position encodings, BERT) of a minibatch on a second
        stream and return a handle for ``forward(batched_inputs, frontend=handle)``.  Nothing in it depends on the
        trainable weights, so a trainer can queue the next minibatch's front end while the current step's launch-bound
        phases (fusion blocks, decoder, criterion, backward) leave most of the GPU idle.  The work per step is the
        same; only its place in time changes."""
        assert self.can_prefetch_frontend()
        dev = self.device if isinstance(self.device, torch.device) else torch.device(self.device)
        cur = torch.cuda.current_stream(dev)
        if self._prefetch_stream is None:
            # default (= lowest) priority.  Measured: a high-priority prefetch stream costs 20 % (36 vs 45 images/s), and
            # putting the step itself on a high-priority stream instead loses as well (39-40)
            self._prefetch_stream = torch.cuda.Stream(device=dev)
        side = self._prefetch_stream
        side.wait_stream(cur)          # (the inputs may have been produced on the current stream)
        with torch.cuda.stream(side), torch.no_grad():
            images, samples = self._canvas_batch(batched_inputs) if self._canvas_sizes is not None else (None, None)
            if samples is None:
                images = self.preprocess_image(batched_inputs)
                samples = nested_tensor_from_tensor_list(images)
            captions, names_list = self._captions(batched_inputs)
            overlap, self.overlap_text_and_image = self.overlap_text_and_image, False   # already off the main stream
            try:
                finish_text, cate_list = self.encode_text(captions, samples.device, defer=True, hidden_only=True,
                                                          **self._prompt_names(names_list))
            finally:
                self.overlap_text_and_image = overlap
            features, poss = self.run_backbone(samples)
            done = torch.cuda.Event()
            done.record(side)
        return {"inputs": batched_inputs, "images": images, "samples": samples, "names_list": names_list,
                "finish_text": finish_text, "cate_list": cate_list, "features": features, "poss": poss, "done": done,
                "stream": side}

    def forward_grounding(self, batched_inputs):
        """The free-text surface (reference GroundingDINO.forward, what ``predict`` reads): ``{"pred_logits": token logits
        [B, Q, max_text_len], "pred_boxes": [B, Q, 4]}`` of the last decoder layer -- ``class_embed(hs, text_dict)`` without the
        fold into category logits, padded with -inf as ``ContrastiveEmbed`` pads.  Eval mode; every input carries its own
        ``"captions"`` string.  ``grounding.predict`` is the tail on top of it."""
        assert not self.training, "forward_grounding is an eval-mode path"
        return self.forward(batched_inputs, grounding=True)

    def forward(self, batched_inputs, frontend=None, grounding=False, **kw):
        if frontend is not None and frontend["inputs"] is batched_inputs:
            cur = torch.cuda.current_stream(frontend["samples"].tensors.device)
            cur.wait_event(frontend["done"])
            images, samples, names_list = frontend["images"], frontend["samples"], frontend["names_list"]
            features, poss, cate_to_token_mask_list = frontend["features"], frontend["poss"], frontend["cate_list"]
            for t in [samples.tensors, samples.mask] + [f.tensors for f in features] + [f.mask for f in features] + list(poss):
                if torch.is_tensor(t):
                    t.record_stream(cur)
            targets = None
            if self.training:
                gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
                targets = self.prepare_targets(gt_instances, cate_to_token_mask_list, names_list)
            text_dict, cate_to_token_mask_list, loss_linear_adapter = frontend["finish_text"]()
            return self._forward_rest(batched_inputs, images, samples, features, poss, text_dict, cate_to_token_mask_list,
                                      loss_linear_adapter, targets, grounding)
        if self._prefetch_stream is not None:
            # A prefetch that this call does not consume (a handle for another minibatch) may still be running: it
            # replays the SAME front-end graphs, whose static input / output buffers this call is about to use.
            torch.cuda.current_stream(self._prefetch_stream.device).wait_stream(self._prefetch_stream)
        images, samples = self._canvas_batch(batched_inputs) if self._canvas_sizes is not None else (None, None)
        if samples is None:
            images = self.preprocess_image(batched_inputs)
            samples = nested_tensor_from_tensor_list(images)
        captions, names_list = self._captions(batched_inputs)
        if self.category_chunk_size is not None and not self.training and not grounding:
            chunks = self._category_chunks(names_list)
            if len(chunks) > 1:      # (a list that is one chunk takes the path below, with its own caption)
                return self._forward_chunked(batched_inputs, images, samples, chunks)
        finish_text, cate_to_token_mask_list = self.encode_text(captions, samples.device, defer=True,
                                                                **({} if grounding else self._prompt_names(names_list)))

        targets = None
        if self.training:
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
            targets = self.prepare_targets(gt_instances, cate_to_token_mask_list, names_list)

        features, poss = self.run_backbone(samples)
        text_dict, cate_to_token_mask_list, loss_linear_adapter = finish_text()
        return self._forward_rest(batched_inputs, images, samples, features, poss, text_dict, cate_to_token_mask_list,
                                  loss_linear_adapter, targets, grounding)

    def _forward_rest(self, batched_inputs, images, samples, features, poss, text_dict, cate_to_token_mask_list,
                      loss_linear_adapter, targets, grounding=False):
        out_or_loss = self.forward_features(features, poss, samples.mask, text_dict,
                                            cate_to_token_mask_list, loss_linear_adapter, targets,
                                            no_padding=getattr(samples, "no_padding", False), token_logits=grounding)
        if self.training or grounding:
            return out_or_loss
        out = out_or_loss
        return self.postprocess(out["pred_logits"], out["pred_boxes"], batched_inputs, images.image_sizes)

    def postprocess(self, box_cls, box_pred, batched_inputs, image_sizes):
        """The evaluation tail of ``forward`` (reference :589-602): top-k detections per image, rescaled to the
        requested output size, clipped, empty boxes dropped.  With ``nms_threshold_for_evaluation`` set, class-aware NMS
        (nms.py) of what is left, in the same order."""
        from . import nms, topk
        from .structures import detector_postprocess
        from .transformer import Switches

        k = self.select_box_nums_for_evaluation
        thr = self.nms_threshold_for_evaluation
        if Switches.native_detections and topk.detections_supported(box_cls, box_pred, k):
            # one launch for the batch and one host read (the counts) instead of ~25 launches and a sync per image
            out_sizes = [(inp.get("height", s[0]), inp.get("width", s[1])) for inp, s in zip(batched_inputs, image_sizes)]
            sizes = self._detection_sizes(image_sizes, out_sizes, box_cls.device)
            if sizes is not None:
                return self._padded_instances(*topk.detections(box_cls.sigmoid(), box_pred, k, sizes), out_sizes)
        results = self.dt_inference(box_cls, box_pred, image_sizes)
        processed = []
        for r, inp, image_size in zip(results, batched_inputs, image_sizes):
            height, width = inp.get("height", image_size[0]), inp.get("width", image_size[1])
            r = detector_postprocess(r, height, width)
            if thr is not None and len(r):
                keep, n_nms = nms.nms_reference(r.pred_boxes.tensor[None], r.scores[None], r.pred_classes[None], None, thr)
                r = r[keep[0, :int(n_nms[0])].to(torch.int64)]
            processed.append({"instances": r})
        return processed

    def _padded_instances(self, scores, labels, xyxy, n_keep, out_sizes):
        """``Instances`` per image from the padded outputs of ``topk.detections`` / ``vocab.merge_detections`` and their
        counts, behind class-aware NMS where ``nms_threshold_for_evaluation`` is set.  One host read, of the counts."""
        from . import nms

        thr = self.nms_threshold_for_evaluation
        if thr is None:
            return [{"instances": Instances(osize, pred_boxes=Boxes(xyxy[b, :n]), scores=scores[b, :n],
                                            pred_classes=labels[b, :n])}
                    for b, (n, osize) in enumerate(zip(n_keep.tolist(), out_sizes))]
        # the suppression reads the counts on the device; the one host read is of the counts behind it
        keep, n_nms = nms.nms_padded(xyxy, scores, labels, n_keep, thr)
        processed = []
        for b, (n, osize) in enumerate(zip(n_nms.tolist(), out_sizes)):
            idx = keep[b, :n].to(torch.int64)
            processed.append({"instances": Instances(osize, pred_boxes=Boxes(xyxy[b][idx]), scores=scores[b][idx],
                                                     pred_classes=labels[b][idx])})
        return processed

    def _category_chunks(self, names_list):
        """The batch's one category list in chunks that fit ``max_text_len`` (vocab.split_categories), remembered per list."""
        from . import vocab

        names = list(names_list[0])
        if any(list(other) != names for other in names_list[1:]):
            raise ValueError("category_chunk_size: the images of a batch must share one category list")
        size = self.category_chunk_size
        if not (size == "auto" or (isinstance(size, int) and not isinstance(size, bool) and size >= 1)):
            raise ValueError("category_chunk_size is None, \"auto\" or a positive int, not %r" % (size,))
        key = ("category_chunks", tuple(names), size, self.max_text_len)
        chunks = self._text_cache.get(key)
        if chunks is None:
            if len(self._text_cache) >= 64:
                self._text_cache.clear()
            chunks = self._text_cache[key] = vocab.split_categories(names, self.tokenizer, self.max_text_len,
                                                                    None if size == "auto" else size)
        return chunks

    def _forward_chunked(self, batched_inputs, images, samples, chunks):
        """Eval-mode ``forward`` for a category list of several chunks: the backbone once; per chunk the text side, the
        transformer, the heads and the chunk's own top-k (``topk.topk_rows``), whose values and flat indices go into the
        chunk's slice of the candidate row -- the chunk's [B, Q, C_j] tensor is dead before the next chunk runs; then ONE
        ``vocab.merge_detections`` call (the global top-k, global labels, the evaluation tail) and the tail of
        ``postprocess``.  No host read per chunk."""
        from . import topk, vocab

        features, poss = self.run_backbone(samples)
        dev, B, k = samples.device, len(batched_inputs), self.select_box_nums_for_evaluation
        no_padding = getattr(samples, "no_padding", False)
        cand_scores = cand_index = boxes = None
        start, classes, offsets = [0], [], []
        for j, chunk in enumerate(chunks):
            text_dict, cate_to_token_mask_list, loss_linear_adapter = self.encode_text([vocab.caption_of(chunk)] * B, dev,
                                                                                       **self._prompt_names([list(chunk)] * B))
            out = self.forward_features(features, poss, samples.mask, text_dict, cate_to_token_mask_list, loss_linear_adapter,
                                        None, no_padding=no_padding)
            C = len(chunk)
            prob = out["pred_logits"][..., :C].sigmoid()
            Q = prob.shape[1]
            if boxes is None:       # every chunk's slice is exactly min(k, Q * C_j) wide: no padding positions
                widths = [min(k, Q * len(c)) for c in chunks]
                for w in widths:
                    start.append(start[-1] + w)
                cand_scores = torch.empty((B, start[-1]), dtype=prob.dtype, device=prob.device)
                cand_index = torch.empty((B, start[-1]), dtype=torch.int64, device=prob.device)
                boxes = torch.empty((len(chunks), B, Q, 4), dtype=out["pred_boxes"].dtype, device=prob.device)
            val, idx = topk.topk_rows(prob.reshape(B, Q * C), widths[j])
            cand_scores[:, start[j]:start[j + 1]] = val
            cand_index[:, start[j]:start[j + 1]] = idx
            boxes[j] = out["pred_boxes"]
            offsets.append(sum(classes))
            classes.append(C)
        image_sizes = images.image_sizes
        out_sizes = [(inp.get("height", s[0]), inp.get("width", s[1])) for inp, s in zip(batched_inputs, image_sizes)]
        sizes = self._detection_sizes(image_sizes, out_sizes, boxes.device)
        if sizes is None:           # fp32 cannot hold a size: the definition scales by the Python numbers
            sizes = torch.tensor([[ih, iw, oh, ow] for (ih, iw), (oh, ow) in zip(image_sizes, out_sizes)], dtype=torch.float64)
        merged = vocab.merge_detections(cand_scores, cand_index, start, classes, offsets, boxes, k, sizes)
        return self._padded_instances(*merged, out_sizes)

    def forward_features(self, features, poss, samples_mask, text_dict, cate_to_token_mask_list,
                         loss_linear_adapter=None, targets=None, no_padding=False, token_logits=False):
        """Everything downstream of the frozen backbone / text encoder: input projections with
        the vision side branches, transformer, heads, and in training mode the criterion
        (reference :483-587).  ``features``: list of NestedTensor, ``poss``: their position
        encodings, ``samples_mask``: [B,H,W] padding mask of the input images.  ``token_logits`` (eval mode): the last
        layer's per-token logits and boxes, without the fold into category logits (``forward_grounding``)."""
        assert not (token_logits and self.training), "token logits are an eval-mode output"
        loss_prompt_memory = text_dict.pop("loss_prompt_memory", None)      # (project_text, use_prompt_memory; else absent)
        poss = list(poss)
        srcs, masks, loss_conv_adapter = [], [], None

        def add_zero_loss(z):
            nonlocal loss_conv_adapter
            if z is not None:
                loss_conv_adapter = z if loss_conv_adapter is None else loss_conv_adapter + z

        for l, feat in enumerate(features):
            src, mask = feat.decompose()
            src, z = self._project_level(l, src)
            add_zero_loss(z)
            srcs.append(src)
            masks.append(mask)
        for l in range(len(srcs), self.num_feature_levels):
            inp = features[-1].tensors if l == len(features) else srcs[-1]
            src, z = self._project_level(l, inp)
            add_zero_loss(z)
            mask = F.interpolate(samples_mask[None].float(), size=src.shape[-2:]).to(torch.bool)[0]
            if len(poss) <= l:  # (callers that start at feature level may pass it themselves)
                poss.append(self.backbone[1](NestedTensor(src, mask)).to(src.dtype))
            srcs.append(src)
            masks.append(mask)

        # (capture under autocast needs the weight-cast cache off, as ZiraTrainer sets it: with the cache on, eager launches)
        autocast_cache = torch.is_autocast_enabled("cuda") and torch.is_autocast_cache_enabled()
        adapter_loss = None
        if (self.use_transformer_graph and self.training and srcs[0].is_cuda and not autocast_cache
                and self._frozen(self.transformer) and torch.is_grad_enabled() and not self.use_adapter):
            hs, reference, hs_enc, ref_enc, init_box_proposal = self._graphed_transformer(
                srcs, masks, poss, text_dict, no_padding=no_padding)
        else:
            hs, reference, hs_enc, ref_enc, init_box_proposal, adapter_loss = self.transformer(
                srcs, masks, None, poss, None, None, text_dict, no_padding=no_padding)

        # Heads (reference groundingdino_dual_zero_rep_branch.py:559-583).  The box MLP is shared by
        # the decoder layers and so is the classifier, so all layers go through them as ONE stacked tensor instead
        # of layer by layer -- and in training the encoder proposals with them: through the same call where the
        # classifier is parameter-free (a deep copy computes the same thing), through the encoder's own module where
        # it is trained (use_cls_linear: the copy has weights of its own), joined behind it.
        n_dec = len(hs)
        shared_heads = (all(m is self.bbox_embed[0] for m in self.bbox_embed)
                        and all(m is self.class_embed[0] for m in self.class_embed))
        enc_cls = getattr(self.transformer, "enc_out_class_embed", None)
        linear_head = isinstance(self.class_embed[0], ContrastiveEmbedwithLinear)
        with_enc = (self.training and hs_enc is not None and shared_heads
                    and type(enc_cls) is type(self.class_embed[0])
                    and isinstance(enc_cls, (ContrastiveEmbed, ContrastiveEmbedwithLinear))
                    and enc_cls.max_text_len == self.class_embed[0].max_text_len
                    and hs_enc[-1].shape == hs[0].shape)
        if shared_heads:
            hs_all = torch.stack(list(hs))                                   # [L, B, Q, d]
            ref_all = torch.stack(list(reference[:-1]))
            outputs_coord_list = box_head(self.bbox_embed[0](hs_all), ref_all)
        else:
            outputs_coord_list = []
            for layer_ref_sig, layer_bbox_embed, layer_hs in zip(reference[:-1], self.bbox_embed, hs):
                unsig = layer_bbox_embed(layer_hs) + inverse_sigmoid(layer_ref_sig)
                outputs_coord_list.append(unsig.sigmoid())
            outputs_coord_list = torch.stack(outputs_coord_list)
        if token_logits:
            return {"pred_logits": self.class_embed[-1](hs[-1], text_dict), "pred_boxes": outputs_coord_list[-1]}
        if shared_heads and linear_head:
            # linear + text product + fold into category logits: one node per module (utils.ContrastiveEmbedwithLinear)
            if with_enc and enc_cls is self.class_embed[0]:
                cls_all = enc_cls.category_logits(torch.cat([hs_all, hs_enc[-1][None]]), text_dict, cate_to_token_mask_list, -100.0)
            else:
                cls_all = self.class_embed[0].category_logits(hs_all, text_dict, cate_to_token_mask_list, -100.0)
                if with_enc:
                    cls_enc = enc_cls.category_logits(hs_enc[-1], text_dict, cate_to_token_mask_list, -100.0)
                    cls_all = torch.cat([cls_all, cls_enc[None]])
            outputs_class = cls_all[:n_dec]
        elif shared_heads:
            cls_in = torch.cat([hs_all, hs_enc[-1][None]]) if with_enc else hs_all
            cls_all = recover_to_cls_logits(self.class_embed[0](cls_in, text_dict),
                                            cate_to_token_mask_list, for_fill=-100.0)
            outputs_class = cls_all[:n_dec]
        else:
            outputs_class = torch.stack([
                recover_to_cls_logits(layer_cls_embed(layer_hs, text_dict), cate_to_token_mask_list, for_fill=-100.0)
                for layer_cls_embed, layer_hs in zip(self.class_embed, hs)])
        out = {"pred_logits": outputs_class[-1], "pred_boxes": outputs_coord_list[-1],
               "cate_to_token_mask_list": cate_to_token_mask_list}

        if self.training:
            if self.aux_loss:
                out["aux_outputs"] = [{"pred_logits": a, "pred_boxes": b}
                                      for a, b in zip(outputs_class[:-1], outputs_coord_list[:-1])]
            if hs_enc is not None:
                if with_enc:
                    interm_class = cls_all[n_dec]
                elif isinstance(enc_cls, ContrastiveEmbedwithLinear):
                    interm_class = enc_cls.category_logits(hs_enc[-1], text_dict, cate_to_token_mask_list, -100.0)
                else:
                    interm_class = self.transformer.enc_out_class_embed(hs_enc[-1], text_dict)
                    interm_class = recover_to_cls_logits(interm_class, cate_to_token_mask_list, for_fill=-100.0)
                out["enc_outputs"] = {"pred_logits": interm_class, "pred_boxes": ref_enc[-1]}
            if with_enc and self.aux_loss:     # the criterion takes all 7 sets as stacked tensors
                out["stacked"] = (cls_all, torch.cat([outputs_coord_list, ref_enc[-1][None]]),
                                  ["_%d" % i for i in range(n_dec - 1)] + ["", "_enc"])
            assert targets is not None and self.criterion is not None
            loss_dict = self.criterion(out, targets)
            weight_dict = self.criterion.weight_dict
            total = None
            stacked = getattr(loss_dict, "stacked", None)
            if stacked and all(name + suf in weight_dict for name, (_, sufs) in stacked.items() for suf in sufs):
                # the criterion made its entries from one vector per loss type: weight the vectors (one multiply per
                # type), hand out their elements under the reference's keys, and keep the sum for the trainer
                for name, (vec, sufs) in stacked.items():
                    w = self._loss_weights(name, sufs, weight_dict, vec)
                    weighted = vec * w
                    for s_, suf in enumerate(sufs):
                        loss_dict[name + suf] = weighted[s_]
                    total = weighted.sum() if total is None else total + weighted.sum()
            else:
                for k in loss_dict.keys():
                    if k in weight_dict:
                        loss_dict[k] = loss_dict[k] * weight_dict[k]
            if self.use_project_adapter and self.use_zero_inter_loss_for_conv:
                loss_dict["loss_conv_adapter"] = loss_conv_adapter * self.loss_adapter_weight
                total = None if total is None else total + loss_dict["loss_conv_adapter"].reshape(())
            if self.use_cet and self.use_zero_inter_loss:
                key = self._text_loss_name()
                loss_dict[key] = loss_linear_adapter * self.loss_adapter_weight
                total = None if total is None else total + loss_dict[key].reshape(())
            if self.use_cet and self.use_prompt_memory:       # weight 1 (groundingdino_dt.py:649-650)
                if loss_prompt_memory is None:
                    raise RuntimeError("use_prompt_memory: the text side was encoded without the category list (names_list)")
                loss_dict["loss_prompt_memory"] = loss_prompt_memory
                total = None if total is None else total + loss_prompt_memory.reshape(())
            if self.use_adapter and self.use_self_kd:
                loss_dict["loss_adapter"] = adapter_loss * self.loss_adapter_weight
                total = None if total is None else total + loss_dict["loss_adapter"].reshape(())
            if total is not None:
                loss_dict.total = total        # == sum(loss_dict.values()); ZiraTrainer back-propagates this one
            return loss_dict
        return out

    # ---- helpers with the reference's names ---------------------------------------------------
    def prepare_targets(self, targets, cate_to_token_mask_list, names_list):
        new_targets = []
        for t in targets:
            h, w = t.image_size
            scale = self._box_scale(w, h)
            new_targets.append({"labels": t.gt_classes,
                                "boxes": box_xyxy_to_cxcywh(t.gt_boxes.tensor / scale)})
        return new_targets

    def _box_scale(self, w, h):
        key = (int(w), int(h), str(self.device))     # (w, h, w, h) per image size, uploaded once
        t = self._pixel_stats.get(key)
        if t is None:
            t = self._pixel_stats[key] = torch.as_tensor([w, h, w, h], dtype=torch.float, device=self.device)
        return t

    def _detection_sizes(self, image_sizes, out_sizes, device):
        """[B, 4] = (img_h, img_w, out_h, out_w) for ``topk.detections``, uploaded once per distinct tuple of sizes; None
        where fp32 cannot hold a size exactly (the op chain scales by the Python numbers)."""
        rows = tuple((float(ih), float(iw), float(oh), float(ow)) for (ih, iw), (oh, ow) in zip(image_sizes, out_sizes))
        key = ("detection_sizes", rows, str(device))
        t = self._pixel_stats.get(key)
        if t is None:
            t = torch.tensor(rows, dtype=torch.float32)
            if t.double().tolist() != [list(r) for r in rows] or not bool((t > 0).all()):
                return None
            t = self._pixel_stats[key] = t.to(device)
        return t

    def preprocess_image(self, batched_inputs):
        images = [self.normalizer(x["image"].to(self.device)) for x in batched_inputs]
        return ImageList.from_tensors(images)

    def normalizer(self, x):
        # the two constants are uploaded once per device (a host list -> device tensor is a
        # blocking copy: 4 of them per step cost 5 ms of host time here)
        key = (x.device, x.dtype)
        cached = self._pixel_stats.get(key)
        if cached is None:
            cached = self._pixel_stats[key] = (
                torch.tensor(self.pixel_mean, device=x.device, dtype=x.dtype).view(3, 1, 1),
                torch.tensor(self.pixel_std, device=x.device, dtype=x.dtype).view(3, 1, 1))
        return (x - cached[0]) / cached[1]

    def dt_inference(self, box_cls, box_pred, image_sizes):
        """sigmoid -> top-k over (query x class) -> boxes in absolute xyxy (reference :634-675)."""
        assert len(box_cls) == len(image_sizes)
        prob = box_cls.sigmoid()
        scores, topk_indexes = torch.topk(prob.view(box_cls.shape[0], -1),
                                          self.select_box_nums_for_evaluation, dim=1)
        topk_boxes = torch.div(topk_indexes, box_cls.shape[2], rounding_mode="floor")
        labels = topk_indexes % box_cls.shape[2]
        boxes = torch.gather(box_pred, 1, topk_boxes.unsqueeze(-1).repeat(1, 1, 4))
        results = []
        for s, lab, b, image_size in zip(scores, labels, boxes, image_sizes):
            r = Instances(image_size)
            r.pred_boxes = Boxes(box_cxcywh_to_xyxy(b))
            r.pred_boxes.scale(scale_x=image_size[1], scale_y=image_size[0])
            r.scores = s
            r.pred_classes = lab
            results.append(r)
        return results

    def unfreeze_module_(self, pat_names, verbose=False):
        for name, param in self.named_parameters():
            if any(p in name for p in pat_names):
                param.requires_grad = True
                if verbose:
                    print("unfreeze:", name)

    def load_state_dict(self, state_dict, strict=True):
        self._replay_cache = None      # (the kept BERT states of replay_memory depend on the weights)
        for k, v in state_dict.items():
            if "prompt_memory_pool" in k:
                class_name = k.split(".")[-1]
                if class_name == "prompt_memory_pool":
                    continue
                # (use_prompt_memory without use_prompt_tuning: the entries are memory, not parameters to train)
                self.prompt_memory_pool[class_name] = nn.Parameter(v, requires_grad=self._pool_trains())
                self.learned_classes.append(class_name[1:-1])
                self._prompt_tables.clear()
                self._replay_cache = None
        return super().load_state_dict(state_dict=state_dict, strict=strict)

    def add_cls_prompt(self, class_names, device=None, fixed_name=False):
        """Pool entries for ``class_names``; entries that exist are kept.  Without ``use_prompt_tuning`` and
        ``use_prompt_memory`` an entry is a random ``[hidden_dim]`` vector on ``device`` (default "cpu") that nothing reads.  With
        either (the sibling class's groundingdino_dt.py:379-437) an entry is ``[n_tok, hidden_dim]``: the class's rows of the
        encoded caption ``".".join(class_names) + "."`` -- with prompt tuning one trained row per token, initialised from what the
        frozen model would have seen; with the prompt memory alone a frozen copy (``requires_grad = False``: memory, not a
        parameter to train, so it stays out of the trainer's bucket and optimizer), taken with the side branch as it stands
        (``ZiraTrainer.after_train`` calls this before the merge, :419-423) -- on ``device`` (default: where the model is).  A
        class whose tokens reach behind ``max_text_len`` raises ``ValueError``."""
        if self.use_prompt_tuning or self.use_prompt_memory:
            return self._add_cls_prompt_rows(list(class_names), device, fixed_name)
        device = "cpu" if device is None else device
        for class_name in class_names:
            self.learned_classes.append(class_name)
            if not fixed_name:
                class_name = "-{}-".format(class_name)
            if class_name not in self.prompt_memory_pool:
                self.prompt_memory_pool[class_name] = nn.Parameter(torch.randn(self.hidden_dim).to(device))

    def _add_cls_prompt_rows(self, class_names, device, fixed_name):
        self.learned_classes.extend(class_names)
        self._prompt_tables.clear()
        self._replay_cache = None
        if not class_names:
            return
        model_device = next(self.parameters()).device
        with torch.no_grad():       # one text pass, no substitution (no category list is handed in)
            text_dict, cate_to_token_mask_list, _ = self.encode_text([".".join(class_names) + "."], model_device)
        encoded_text, masks = text_dict["encoded_text"][0], cate_to_token_mask_list[0]
        T = encoded_text.shape[0]
        if masks.shape[0] != len(class_names):
            raise ValueError("add_cls_prompt: the caption of %d class names tokenises into %d categories (an empty name, or one "
                             "holding a separator?)" % (len(class_names), masks.shape[0]))
        masks = masks.to("cpu")       # the one host read; the reference indexes with the masks, which reads them too
        for class_name, mask in zip(class_names, masks):
            if bool(mask[T:].any()) or not bool(mask.any()):
                raise ValueError("add_cls_prompt: class %r has %s: it gets no prompt" % (
                    class_name, "tokens behind max_text_len = %d" % self.max_text_len if bool(mask.any()) else "no tokens"))
        for class_name, mask in zip(class_names, masks):       # (nothing is created where a class raises)
            key = class_name if fixed_name else "-{}-".format(class_name)
            if key not in self.prompt_memory_pool:
                rows = encoded_text[mask[:T].to(encoded_text.device)].detach().clone()
                self.prompt_memory_pool[key] = nn.Parameter(rows.to(model_device if device is None else device),
                                                            requires_grad=self._pool_trains())

    def _pool_trains(self):
        """Pool entries are trained parameters except under ``use_prompt_memory`` alone, where they are stored memory."""
        return self.use_prompt_tuning or not self.use_prompt_memory

    def before_train(self):
        """Freeze everything, then unfreeze what the method trains: every parameter whose name
        contains "adapter" -- the two side branches and their twins -- and what the baselines' switches name
        (reference :722-734)."""
        if self.freeze_all:
            for param in self.parameters():
                param.requires_grad = False
        if self.use_bert_tuning:
            self.unfreeze_module_(["bert", "feat_map"])
        if self.use_cls_linear:      # linear probing: both heads are trained, the encoder's copies with them (reference :728-729)
            self.unfreeze_module_(["class_embed", "bbox_embed"])
        if self.use_prompt_tuning:
            self.unfreeze_module_(["prompt_memory_pool"])
        if self.use_project_tuning:
            self.unfreeze_module_(["input_proj"])
        self.unfreeze_module_(["adapter"])

    def after_train(self):
        """End of a task: merge every side branch into its twin (reference :739-745)."""
        for module in self.modules():
            if hasattr(module, "__rep__"):
                module.__rep__()

    def replay_parameter_prefixes(self):
        """Name prefixes of the parameters ``replay_memory``'s losses reach: the language side branch with its twin, and -- where
        their switches make them trainable -- the text encoder, ``feat_map`` and the pool entries."""
        branch = "rep_language_adapter." if self.side_branch == "multilayer" else "rep_linear_adapter."
        if self.text_branch == "cet":
            branch = "cet_adapter."
        return (branch, "bert.", "feat_map.", "prompt_memory_pool.")

    def _text_loss_name(self):
        """The loss dict's key of the text side's zero-interference term: the reference's name for the module that is built."""
        if self.text_branch == "cet":
            return "loss_adapter_text"
        return "loss_language_adapter" if self.side_branch == "multilayer" else "loss_linear_adapter"

    def replay_memory(self):
        """One iteration's losses of the text-only replay stage (groundingdino_dt.py ``replay_memory`` :786-838; it takes no
        images): the captions of all learned classes are encoded -- feat_map + side branch -- and pulled back to the stored rows.
        Returns ``{"loss_prompt_memory": 0.5 * loss}`` and, with ``use_zero_inter_loss``, the side branch's zero-interference
        term times ``loss_adapter_weight`` under the key the training forward uses for it (``loss_linear_adapter`` /
        ``loss_language_adapter``; with ``text_branch="cet"``, the module the reference's name belongs to, ``loss_adapter_text``).

        The captions are ``vocab.split_categories(learned_classes)``: J = 1 is the reference's single caption
        ``".".join(learned) + "."``; J > 1 -- a departure -- is this package's answer to lists longer than ``max_text_len``,
        which the reference feeds to BERT uncut; they are encoded as one batch of J rows.  A class listed twice in
        ``learned_classes`` is replayed once.  With BERT frozen its states for these captions are constant: they are computed
        once per (learned classes, device) and kept, so an iteration is ``project_text`` + the loss."""
        from . import vocab

        if not (self.use_cet and self.use_prompt_memory and self.training):
            raise RuntimeError("replay_memory needs use_cet and use_prompt_memory, in training mode")
        learned = list(dict.fromkeys(self.learned_classes))
        if not learned:
            raise RuntimeError("replay_memory: learned_classes is empty -- nothing was stored to replay")
        missing = [c for c in learned if "-{}-".format(c) not in self.prompt_memory_pool]
        if missing:
            raise KeyError("replay_memory: learned classes without a pool entry: %s" % ", ".join(missing))
        device = next(self.parameters()).device
        key = (tuple(learned), str(device), self.max_text_len)
        cached = self._replay_cache
        if cached is None or cached[0] != key:
            chunks = vocab.split_categories(learned, self.tokenizer, self.max_text_len)
            cached = self._replay_cache = [key, [vocab.caption_of(c) for c in chunks], [list(c) for c in chunks], None]
        _, captions, names_list, hidden = cached
        frozen = self._frozen(self.bert)
        if not frozen:
            hidden = cached[3] = None      # (a trained BERT's states change; none are kept, also for when it is frozen again)
        elif hidden is None:
            with torch.no_grad():
                hidden = cached[3] = self._bert_hidden(dict(self._encoder_inputs(captions, device)[4]))
        text_dict, _, loss_linear_adapter = self.encode_text(captions, device, names_list=names_list, bert_hidden=hidden)
        losses = {"loss_prompt_memory": text_dict.pop("loss_prompt_memory") * 0.5}
        if self.use_zero_inter_loss:
            losses[self._text_loss_name()] = loss_linear_adapter.reshape(()) * self.loss_adapter_weight
        return losses

    def side_branch_parameters(self):
        """The only tensors that ever receive gradients in ZiRa (4 622 853 values for Swin-T)."""
        return [p for n, p in self.named_parameters() if "adapter" in n]


@MODULE_BUILD_FUNCS.registe_with_name(module_name="dualzerorepbranchgroundingdino")
def build_dual_zero_rep_branch_groundingdino(args, bert=None, tokenizer=None, side_branch="rep", **model_kw):
    backbone = build_backbone(args)
    transformer = build_transformer(args)
    criterion = build_criterion(args)
    return GroundingDINO(
        backbone, transformer, num_queries=args.num_queries, aux_loss=True, iter_update=True,
        query_dim=4, num_feature_levels=args.num_feature_levels, nheads=args.nheads,
        dec_pred_bbox_embed_share=args.dec_pred_bbox_embed_share, two_stage_type=args.two_stage_type,
        two_stage_bbox_embed_share=args.two_stage_bbox_embed_share,
        two_stage_class_embed_share=args.two_stage_class_embed_share, num_patterns=args.num_patterns,
        dn_number=0, dn_box_noise_scale=args.dn_box_noise_scale,
        dn_label_noise_ratio=args.dn_label_noise_ratio, dn_labelbook_size=args.dn_labelbook_size,
        text_encoder_type=args.text_encoder_type, sub_sentence_present=args.sub_sentence_present,
        max_text_len=args.max_text_len, criterion=criterion, freeze_all=args.freeze_all,
        select_box_nums_for_evaluation=args.select_box_nums_for_evaluation,
        loss_adapter_weight=args.loss_adapter_weight, use_cet=args.use_cet,
        use_prompt_memory=args.use_prompt_memory, use_zero_inter_loss=args.use_zero_inter_loss,
        use_add_names=args.use_add_names, use_bert_tuning=args.use_bert_tuning,
        use_cls_linear=args.use_cls_linear, use_prompt_tuning=args.use_prompt_tuning,
        use_prompt_memory_output=args.use_prompt_memory_output,
        use_project_tuning=getattr(args, "use_project_tuning", False),
        use_project_adapter=model_kw.pop("use_project_adapter", args.use_project_adapter),
        use_zero_inter_loss_for_conv=args.use_zero_inter_loss_for_conv,
        use_learned_names=args.use_learned_names, device=getattr(args, "device", "cuda"),
        bert=bert, tokenizer=tokenizer, side_branch=side_branch, use_adapter=getattr(args, "use_adapter", False),
        use_self_kd=getattr(args, "use_self_kd", False),
        text_branch=model_kw.pop("text_branch", getattr(args, "text_branch", "rep")),
        lora_down_dim=getattr(args, "lora_down_dim", None), **model_kw)


@MODULE_BUILD_FUNCS.registe_with_name(module_name="dtgroundingdino")
def build_dt_groundingdino(args, bert=None, tokenizer=None):
    """The CET text-adapter baseline (reference groundingdino_dt.py, builder :1036-1110, run with
    ``GroundingDINO_SwinT_OGC_dt.py``): the same detector with ``text_branch="cet"`` -- ``use_cet`` builds ``cet_adapter``
    (``args.cet_type``, ``args.cet_middle_dim``; defaults "Adapter" and 1024) in place of the language ``RepZeroLinear`` -- and no
    vision side branches.  Departures from groundingdino_dt.py, all stated:

    * the text side's zero-interference term stands in the loss dict under its own key, ``loss_adapter_text`` (the name the
      reference's ``replay_memory`` gives it), times ``loss_adapter_weight``; the reference's training forward adds it to the
      transformer's adapter loss and reports the sum as ``loss_adapter`` (:647-654).  ``loss_adapter`` here stays the
      transformer's own, under ``use_adapter`` and ``use_self_kd``;
    * ``use_project_adapter`` is off whatever ``args`` says: the dt class's optional branches beside the input projections are
      plain convolutions with a GroupNorm (:256-279), modules this package does not build; its builder defaults to none;
    * the memory loss is the L1 mean whatever ``zero_loss_type`` (the reference applies the selected ``adapter_loss`` to it as
      well, :519); ``use_prompt_memory`` with another type raises;
    * ``cet_type="Transformer"`` raises ``NotImplementedError``; ``load_state_dict`` does not re-run ``add_cls_prompt`` or the
      freezing (:761-784): pool entries load as they are and ``before_train`` freezes, as in the class this package mirrors;
    * denoising queries (``dn_number``) are off, as in every builder here, and ``inference`` / ``add_cls_prompt``'s eval path
      (:840-1033) is this class's ordinary eval forward.

    ``after_train`` has nothing to merge for ``cet_adapter``: its keys stay in the final checkpoint."""
    return build_dual_zero_rep_branch_groundingdino(
        args, bert=bert, tokenizer=tokenizer, text_branch="cet", cet_type=getattr(args, "cet_type", "Adapter"),
        cet_middle_dim=getattr(args, "cet_middle_dim", 1024), zero_loss_type=getattr(args, "zero_loss_type", "L1"),
        use_project_adapter=False)


@MODULE_BUILD_FUNCS.registe_with_name(module_name="dualzerorepmultilayerbranchgroundingdino")
def build_dual_zero_rep_multi_layer_branch_groundingdino(args, bert=None, tokenizer=None):
    """The multilayer-branch ablation (reference groundingdino_dual_zero_rep_multilayer_branch.py:971-1020):
    same constructor arguments, other side-branch modules (rsb_multilayer.py)."""
    model = build_dual_zero_rep_branch_groundingdino(args, bert=bert, tokenizer=tokenizer, side_branch="multilayer")
    return model


def build_model(args, **kw):
    """groundingdino/models/__init__.py:11-18: dispatch on ``args.modelname``."""
    assert args.modelname in MODULE_BUILD_FUNCS, "unknown model %s" % args.modelname
    return MODULE_BUILD_FUNCS.get(args.modelname)(args, **kw)
