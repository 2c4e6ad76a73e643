"""Phrase grounding scored on the device: Flickr30k-Entities-style Recall@k and RefCOCO-style top-1 Precision@IoU for what
``GroundingDINO.forward_grounding`` returns.  The reference has no evaluator of this kind, so the definition is written down here
(and, for the C ABI, in include/zira_phrase.h):

- the score of a query for a phrase is the MAXIMUM of its token probabilities over the phrase's tokens -- the ``predict`` tail's
  rule restricted to the phrase, not a mean over a normalised positive map; a NaN among them makes the score NaN;
- the queries are ranked by the project's one stable descending order (``topk.topk_rows``; NaN first, ties by query index) and
  the first ``min(k_max, Q)`` are the candidates; their boxes go to absolute xyxy by the detections tail's arithmetic with the
  output frame equal to ``sizes`` (clipped; a NaN coordinate clips to 0);
- IoU in fp64, ``inter / union`` with no ``+ 1``; a hit is ``iou >= thr`` against ANY ground-truth box of the phrase, or with
  ``merged=True`` against their one union box (the "merged boxes" protocol);
- a phrase with no token bit below T or with no ground-truth box is not valid: it is counted neither as a hit nor as a miss.

``match`` is one launch for the batch (csrc/phrasematch.hip), without a host read; ``match_reference`` is the same function as
torch ops on the tensors' own device, for CPU tensors, other dtypes, shapes outside the kernel's limits and the tests.
``PhraseGroundingEvaluator`` keeps two small integer tensors where the outputs are and reads them once, in ``evaluate()``;
``inference_on_grounding_dataset`` is ``box_eval.run_dataset``, the loop of the box evaluators.

Mask words are int32 tensors that hold the 32 bits of a uint32 word: token ``t`` at bit ``t % 32`` of word ``t // 32``, the layout
of ``grounding.Grounded.token_bits``."""
import ctypes
import re
from collections import namedtuple

import torch

from . import _lib, box_eval
from . import grounding

MAX_B, MAX_Q, MAX_T, MAX_P, MAX_G, MAX_K, MAX_THRS = (_lib.PHRASE_CONSTANTS["ZIRA_PHRASE_MAX_" + k]
                                                      for k in ("B", "Q", "T", "P", "G", "K", "THRS"))
FORCE_REFERENCE = False     # True: ``match`` is ``match_reference`` (tests, A/B)

# top_query [B, P, k_max] int32 (-1 behind the candidates), top_score [B, P, k_max] fp32, top_iou [B, P, k_max] fp64 (both 0 behind
# them), first_hit [B, P, N_thr] int32 (k_max: no hit), valid [B, P] uint8; a phrase that is not valid holds -1 / 0 / 0 / k_max
PhraseMatch = namedtuple("PhraseMatch", "top_query top_score top_iou first_hit valid")
_DTYPES = (torch.float32, torch.float32, torch.float32, torch.int32, torch.float32, torch.int32)


def _shapes_ok(t) -> bool:
    prob, boxes, sizes, phrase_bits, gt_boxes, gt_count = t
    if not all(torch.is_tensor(x) for x in t) or prob.dim() != 3 or phrase_bits.dim() != 3 or gt_boxes.dim() != 4:
        return False
    (B, Q, T), P, G = prob.shape, phrase_bits.shape[1], gt_boxes.shape[2]
    want = ((B, Q, T), (B, Q, 4), (B, 2), (B, P, (T + 31) // 32), (B, P, G, 4), (B, P))
    return B >= 1 and Q >= 1 and T >= 1 and all(tuple(x.shape) == s for x, s in zip(t, want))


def _params(k_max, iou_thrs):
    k_max, thrs = int(k_max), tuple(float(t) for t in iou_thrs)
    if k_max < 1 or not thrs:
        raise ValueError("phrase matching: k_max >= 1 and at least one IoU threshold")
    return k_max, thrs


def match_supported(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, k_max=10, iou_thrs=(0.5,), merged=False) -> bool:
    """True where ``match`` runs the kernel: contiguous tensors of the entry's dtypes on one GPU, inside its limits."""
    t = (prob, boxes, sizes, phrase_bits, gt_boxes, gt_count)
    if FORCE_REFERENCE or not _shapes_ok(t) or not prob.is_cuda:
        return False
    if not all(x.dtype == d and x.device == prob.device and x.is_contiguous() for x, d in zip(t, _DTYPES)):
        return False
    (B, Q, T), P, G = prob.shape, phrase_bits.shape[1], gt_boxes.shape[2]
    return (B <= MAX_B and Q <= MAX_Q and T <= MAX_T and 1 <= P <= MAX_P and 1 <= G <= MAX_G and 1 <= int(k_max) <= MAX_K
            and 1 <= len(tuple(iou_thrs)) <= MAX_THRS)


def _launch(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, k_max, thrs, merged):
    """``zira_phrase_match_f32`` on the current stream: one launch, nothing uploaded, the host never waits; capturable."""
    (B, Q, T), P, G, N = prob.shape, phrase_bits.shape[1], gt_boxes.shape[2], len(thrs)
    lib = _lib.load()
    if lib.zira_phrase_match_lds_bytes(Q, T, G, k_max, N) == 0:
        raise RuntimeError("zira_phrase_match_f32 does not serve Q=%d T=%d G=%d k_max=%d thresholds=%d" % (Q, T, G, k_max, N))
    dev = prob.device
    out = PhraseMatch(torch.empty((B, P, k_max), dtype=torch.int32, device=dev),
                      torch.empty((B, P, k_max), dtype=torch.float32, device=dev),
                      torch.empty((B, P, k_max), dtype=torch.float64, device=dev),
                      torch.empty((B, P, N), dtype=torch.int32, device=dev), torch.empty((B, P), dtype=torch.uint8, device=dev))
    c_thrs = (ctypes.c_double * N)(*thrs)
    with torch.cuda.device(dev):
        rc = lib.zira_phrase_match_f32(prob.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), phrase_bits.data_ptr(),
                                       gt_boxes.data_ptr(), gt_count.data_ptr(), B, Q, T, P, G, k_max, c_thrs, N, int(bool(merged)),
                                       out.top_query.data_ptr(), out.top_score.data_ptr(), out.top_iou.data_ptr(),
                                       out.first_hit.data_ptr(), out.valid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_phrase_match_f32 failed: hipError %d" % rc)
    return out


def match(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, k_max=10, iou_thrs=(0.5,), merged=False):
    """prob [B, Q, T] and boxes [B, Q, 4] (normalised cxcywh) as ``forward_grounding`` gives them, sizes [B, 2] = (h, w) of the
    frame of the ground truth, phrase_bits [B, P, ceil(T / 32)] int32, gt_boxes [B, P, G, 4] absolute xyxy, gt_count [B, P] int32
    -> ``PhraseMatch``.  On a GPU one launch on the current stream, without a host read or a global atomic, capturable; what
    ``match_supported`` declines (CPU tensors, other dtypes, shapes outside the limits, ``FORCE_REFERENCE``) takes
    ``match_reference``."""
    k_max, thrs = _params(k_max, iou_thrs)
    args = (prob, boxes, sizes, phrase_bits, gt_boxes, gt_count)
    if not match_supported(*args, k_max, thrs, merged):
        return match_reference(*args, k_max, thrs, merged)
    return _launch(*(x.detach() for x in args), k_max, thrs, merged)


def match_reference(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, k_max=10, iou_thrs=(0.5,), merged=False):
    """The definition (module docstring), as torch ops on the tensors' own device.  Floating inputs of another dtype are taken
    as fp32, integer ones as int32.  The scores are formed one phrase at a time; everything behind them for the batch at once."""
    t = (prob, boxes, sizes, phrase_bits, gt_boxes, gt_count)
    if not _shapes_ok(t):
        raise ValueError("match_reference: prob [B, Q, T], boxes [B, Q, 4], sizes [B, 2], phrase_bits [B, P, ceil(T / 32)], "
                         "gt_boxes [B, P, G, 4], gt_count [B, P]")
    K, thrs = _params(k_max, iou_thrs)
    prob, boxes, sizes, gt_boxes = (x.detach().to(torch.float32) for x in (prob, boxes, sizes, gt_boxes))
    (B, Q, T), P, G, N = prob.shape, phrase_bits.shape[1], gt_boxes.shape[2], len(thrs)
    kc, dev = min(K, Q), prob.device
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)

    tok = torch.arange(T, device=dev)
    words = phrase_bits.detach().to(torch.int64) & 0xFFFFFFFF
    token_mask = ((words[:, :, tok >> 5] >> (tok & 31)) & 1).bool()                            # [B, P, T]
    count = gt_count.detach().to(torch.int64).clamp(0, G)
    valid = token_mask.any(-1) & (count > 0)

    # ---- scores and ranking
    score = torch.empty((B, P, Q), dtype=torch.float32, device=dev)
    below = f32(float("-inf"))
    for p in range(P):
        score[:, p] = torch.where(token_mask[:, p, None, :], prob, below).amax(dim=-1)
    score = torch.where(torch.isnan(score), f32(float("nan")), score + 0.0)                    # one NaN, one zero
    order = torch.sort(score, dim=-1, descending=True, stable=True).indices[..., :kc]          # [B, P, kc]
    top_score = torch.gather(score, -1, order)

    # ---- candidate boxes: the detections tail's chain with the output frame equal to the image frame (scale 1)
    cx, cy, bw, bh = boxes[torch.arange(B, device=dev)[:, None, None], order].unbind(-1)       # [B, P, kc] each
    img_h, img_w = sizes[:, 0].view(B, 1, 1), sizes[:, 1].view(B, 1, 1)
    half_w, half_h = 0.5 * bw, 0.5 * bh
    clip = lambda x, hi: torch.fmin(torch.fmax(x, f32(0.0)), hi)                               # C's fmaxf / fminf: NaN -> 0
    x0, x1 = clip((cx - half_w) * img_w, img_w), clip((cx + half_w) * img_w, img_w)
    y0, y1 = clip((cy - half_h) * img_h, img_h), clip((cy + half_h) * img_h, img_h)

    # ---- ground truth: the first gt_count boxes, or their union
    real = torch.arange(G, device=dev) < count[..., None]                                      # [B, P, G]
    gt = gt_boxes
    if merged and G > 0:
        isnan = torch.isnan(gt) | ~real[..., None]
        lo = torch.where(isnan, f32(float("inf")), gt).amin(dim=2)
        hi = torch.where(isnan, f32(float("-inf")), gt).amax(dim=2)
        union = torch.where(isnan.all(dim=2), f32(float("nan")), torch.cat([lo[..., :2], hi[..., 2:]], -1))   # fminf / fmaxf
        gt, real = union[:, :, None, :], (count > 0)[..., None]
    d = lambda v: v.to(torch.float64)[..., None]                                               # [B, P, kc, 1]
    g = lambda i: gt[..., i].to(torch.float64)[:, :, None, :]                                  # [B, P, 1, G]
    x0, y0, x1, y1 = d(x0), d(y0), d(x1), d(y1)
    gx0, gy0, gx1, gy1 = g(0), g(1), g(2), g(3)
    area, gt_area = (x1 - x0) * (y1 - y0), (gx1 - gx0) * (gy1 - gy0)
    w, h = torch.fmin(x1, gx1) - torch.fmax(x0, gx0), torch.fmin(y1, gy1) - torch.fmax(y0, gy0)
    inter = w * h
    quotient = inter / (area + gt_area - inter)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    iou = torch.where((w > 0) & (h > 0) & ~torch.isnan(quotient) & real[:, :, None, :], quotient, zero)
    top_iou = iou.amax(dim=-1) if iou.shape[-1] else zero.expand(B, P, kc)                     # [B, P, kc]

    # ---- the first hit per threshold
    thr = torch.tensor(thrs, dtype=torch.float64, device=dev)
    ranks = torch.arange(kc, dtype=torch.int32, device=dev)[:, None]
    none = torch.tensor(K, dtype=torch.int32, device=dev)
    first_hit = torch.where(top_iou[..., None] >= thr, ranks, none).amin(dim=2)                # [B, P, N]

    out = PhraseMatch(torch.full((B, P, K), -1, dtype=torch.int32, device=dev), torch.zeros((B, P, K), dtype=torch.float32, device=dev),
                      torch.zeros((B, P, K), dtype=torch.float64, device=dev), torch.full((B, P, N), K, dtype=torch.int32, device=dev),
                      valid.to(torch.uint8))
    v = valid[..., None]
    out.top_query[..., :kc] = torch.where(v, order.to(torch.int32), out.top_query[..., :kc])
    out.top_score[..., :kc] = torch.where(v, top_score, out.top_score[..., :kc])
    out.top_iou[..., :kc] = torch.where(v, top_iou, out.top_iou[..., :kc])
    out.first_hit[:] = torch.where(v, first_hit, out.first_hit)
    return out


# ---- the host side: character spans -> mask words ------------------------------------------------------------------------------
class TokenSpans(grounding.WordTable):
    """``grounding.WordTable`` with the character range of every token beside its word: ``offsets[i]`` is ``(begin, end)`` in
    the caption, or None for a token that stands for no text ([CLS], [SEP], padding)."""

    def __init__(self, table, offsets):
        super().__init__(table)
        self.offsets = [None if o is None else (int(o[0]), int(o[1])) for o in offsets]
        if len(self.offsets) != len(self.table):
            raise ValueError("TokenSpans: one character range (or None) per token")


def tokenize_with_offsets(tokenizer, caption) -> TokenSpans:
    """``grounding.tokenize_caption`` plus the tokens' character ranges.  A tokenizer whose output knows them (transformers'
    fast tokenizers: ``token_to_chars``) is asked; ``bert.SimpleTokenizer`` makes one token per run of characters between
    blanks, with "." and "?" tokens of their own, so its ranges are those runs in order."""
    tok = tokenizer([caption], padding="longest", return_tensors="pt")
    if callable(getattr(tok, "token_to_chars", None)) and callable(getattr(tok, "token_to_word", None)):
        n = int(tok["input_ids"].shape[1])
        spans = [tok.token_to_chars(0, i) for i in range(n)]
        return TokenSpans([tok.token_to_word(0, i) for i in range(n)], [None if s is None else (s[0], s[1]) for s in spans])
    table = grounding.tokenize_caption(tokenizer, caption).table
    runs = [m.span() for m in re.finditer(r"[.?]|[^\s.?]+", caption)]
    if len(runs) != sum(word is not None for word in table):
        raise ValueError("tokenize_with_offsets: the tokenizer's tokens are not the caption's runs of characters")
    runs = iter(runs)
    return TokenSpans(table, [None if word is None else next(runs) for word in table])


def phrase_bits_from_spans(tokenized, spans, num_tokens=None):
    """A list of character spans ``[(begin, end), ...]`` per phrase -> the ``[P, ceil(num_tokens / 32)]`` int32 mask words
    ``match`` takes.  ``tokenized``: ``TokenSpans`` (``tokenize_with_offsets``) or a plain list of ``(begin, end)`` / None per
    token.  A token's bit is set when its character range intersects one of the phrase's spans -- a span that cuts a token
    marks it, as the reference's ``create_positive_map_from_span`` marks every token from the span's first character's to its
    last character's.  ``num_tokens`` (default: the tokens there are) is the model's T; tokens at and behind it are dropped, as
    ``encode_text`` cuts the caption."""
    offsets = list(getattr(tokenized, "offsets", tokenized))
    T = len(offsets) if num_tokens is None else int(num_tokens)
    if T < 1:
        raise ValueError("phrase_bits_from_spans: at least one token")
    words = [[0] * ((T + 31) // 32) for _ in spans]
    for row, phrase in zip(words, spans):
        for begin, end in phrase:
            for t, o in enumerate(offsets[:T]):
                if o is not None and o[0] < o[1] and o[0] < end and begin < o[1]:
                    row[t >> 5] |= 1 << (t & 31)
    signed = [[w - (1 << 32) if w >= (1 << 31) else w for w in row] for row in words]          # the uint32 word's bit pattern
    return torch.tensor(signed, dtype=torch.int32).reshape(len(words), (T + 31) // 32)


# ---- the evaluator -----------------------------------------------------------------------------------------------------------
class PhraseGroundingEvaluator:
    """``CocoBoxEvaluator``'s surface (``reset`` / ``process`` / ``merge`` / ``evaluate``) for phrase grounding.  ``process``
    matches the batch in one launch and adds to two integer tensors where the outputs are -- the hit counts ``[len(ks), N_thr]``
    and the number of valid phrases -- with torch ops; nothing is read on the host before ``evaluate()``, which reads them once
    per device and returns ``{"grounding": {...}}`` in percent: ``"R@k"`` with one threshold, ``"R@k/IoU=0.50"`` ... with
    several, ``-1.0`` everywhere when no valid phrase was seen.  Flickr30k-Entities recall is the default; RefCOCO-style
    precision is ``ks=(1,)`` with ``iou_thrs=(0.5, 0.6, 0.7, 0.8, 0.9)``.  ``tokenizer``: needed only where phrases come as
    character spans without a tokenization of their caption."""

    def __init__(self, ks=(1, 5, 10), iou_thrs=(0.5,), merged=False, k_max=None, tokenizer=None):
        self.ks = tuple(int(k) for k in ks)
        self.iou_thrs = tuple(float(t) for t in iou_thrs)
        self.merged = bool(merged)
        if not self.ks or min(self.ks) < 1 or not self.iou_thrs:
            raise ValueError("PhraseGroundingEvaluator: ks >= 1 and at least one IoU threshold")
        self.k_max = max(self.ks) if k_max is None else int(k_max)
        if max(self.ks) > self.k_max:
            raise ValueError("PhraseGroundingEvaluator: k = %d is beyond the k_max = %d candidates that are matched"
                             % (max(self.ks), self.k_max))
        self.tokenizer = tokenizer
        self._ks = {}               # device -> ks as an int32 tensor there (uploaded once)
        self.reset()

    def reset(self):
        self._state = {}            # device -> [hits [len(ks), N_thr] int64, valid phrases [] int64], both on the device

    def process_padded(self, prob, boxes, sizes, phrase_bits, gt_boxes, gt_count):
        """One batch from raw tensors (``match``'s inputs)."""
        m = match(prob, boxes, sizes, phrase_bits, gt_boxes, gt_count, self.k_max, self.iou_thrs, self.merged)
        dev = m.first_hit.device
        ks = self._ks.get(dev)
        if ks is None:
            ks = self._ks[dev] = torch.tensor(self.ks, dtype=torch.int32, device=dev)
        valid = m.valid != 0
        hits = ((m.first_hit[:, :, None, :] < ks[None, None, :, None]) & valid[:, :, None, None]).sum(dim=(0, 1))
        state = self._state.get(dev)
        if state is None:
            self._state[dev] = [hits, valid.sum()]
        else:
            state[0] += hits
            state[1] += valid.sum()
        return m

    def _bits(self, x, T):
        phrases = x["phrases"]
        if torch.is_tensor(phrases):
            if phrases.dim() != 2 or phrases.shape[1] != (T + 31) // 32:
                raise ValueError("process: ready phrase bits are [P, ceil(T / 32)] words")
            return phrases.to(torch.int32).cpu()
        tokenized = x.get("tokenized")
        if tokenized is None:
            if self.tokenizer is None:
                raise ValueError("process: phrases given as character spans need the input's \"tokenized\" or the evaluator's tokenizer")
            tokenized = tokenize_with_offsets(self.tokenizer, x["captions"])
        return phrase_bits_from_spans(tokenized, phrases, T)

    def process(self, inputs, outputs):
        """``inputs``: the batched_inputs dicts, each with ``"phrases"`` -- per phrase a list of character spans ``(begin, end)``
        into the input's ``"captions"`` (tokenized with ``"tokenized"``, a ``TokenSpans``, or the evaluator's tokenizer), or the
        ready ``[P, ceil(T / 32)]`` mask words -- ``"phrase_boxes"``, per phrase its ground-truth boxes ``[n, 4]`` as absolute
        xyxy, and the frame they live in as ``"height"`` / ``"width"`` (default: the image's own).  ``outputs``: what
        ``forward_grounding`` returned."""
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        dev, (B, Q, T) = logits.device, logits.shape
        bits = [self._bits(x, T) for x in inputs]
        gts = [[torch.as_tensor(g, dtype=torch.float32).reshape(-1, 4) for g in x["phrase_boxes"]] for x in inputs]
        if len(inputs) != B or any(len(b) != len(g) for b, g in zip(bits, gts)):
            raise ValueError("process: one input per image, one list of boxes per phrase")
        P = max(1, max(len(b) for b in bits))
        G = max(1, max((len(g) for per in gts for g in per), default=1))
        W = (T + 31) // 32
        phrase_bits = torch.zeros((B, P, W), dtype=torch.int32)
        gt_boxes = torch.zeros((B, P, G, 4), dtype=torch.float32)
        gt_count = torch.zeros((B, P), dtype=torch.int32)
        sizes = torch.zeros((B, 2), dtype=torch.float32)
        for b, x in enumerate(inputs):
            phrase_bits[b, :len(bits[b])] = bits[b]
            for p, g in enumerate(gts[b]):
                gt_boxes[b, p, :len(g)], gt_count[b, p] = g, len(g)
            sizes[b, 0] = float(x["height"] if "height" in x else x["image"].shape[-2])
            sizes[b, 1] = float(x["width"] if "width" in x else x["image"].shape[-1])
        prob = logits.detach().to(torch.float32).sigmoid().contiguous()
        self.process_padded(prob, boxes.detach().to(torch.float32).contiguous(), sizes.to(dev), phrase_bits.to(dev),
                            gt_boxes.to(dev), gt_count.to(dev))

    def merge(self, other):
        """Add another evaluator's counts (a data-parallel run gathers its ranks' evaluators with this).  State on the same
        device is added there; state on another device stays where it is until ``evaluate()``."""
        if (other.ks, other.iou_thrs, other.merged, other.k_max) != (self.ks, self.iou_thrs, self.merged, self.k_max):
            raise ValueError("merge: the evaluators differ in ks, thresholds, k_max or the merged-boxes protocol")
        for dev, (hits, n) in other._state.items():
            if dev in self._state:
                self._state[dev][0] += hits
                self._state[dev][1] += n
            else:
                self._state[dev] = [hits.clone(), n.clone()]
        return self

    def names(self):
        """The result's keys, ``[len(ks)][N_thr]``."""
        if len(self.iou_thrs) == 1:
            return [["R@%d" % k] for k in self.ks]
        return [["R@%d/IoU=%.2f" % (k, t) for t in self.iou_thrs] for k in self.ks]

    def evaluate(self):
        hits = [[0] * len(self.iou_thrs) for _ in self.ks]
        n = 0
        for counts, valid in self._state.values():
            both = torch.cat([counts.reshape(-1), valid.reshape(1)]).cpu().tolist()             # ONE device -> host copy
            n += both[-1]
            for i in range(len(self.ks)):
                for j in range(len(self.iou_thrs)):
                    hits[i][j] += both[i * len(self.iou_thrs) + j]
        self.hits, self.num_valid = hits, n
        return {"grounding": {name: (100.0 * h / n if n > 0 else -1.0)
                              for row, names in zip(hits, self.names()) for h, name in zip(row, names)}}


def inference_on_grounding_dataset(model, loader, evaluator):
    """``evaluation.inference_on_dataset`` for the free-text surface: ``box_eval.run_dataset`` over
    ``model.forward_grounding(inputs)``.  As ``run_task``'s ``evaluate=``:
    ``lambda model, spec: inference_on_grounding_dataset(model, loader, evaluator)``."""
    return box_eval.run_dataset(model, loader, evaluator, lambda inputs: model.forward_grounding(inputs))
