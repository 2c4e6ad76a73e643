"""The free-text grounding tail: a caption in, boxes with the matched phrase out (reference ``predict`` /
``get_phrases_from_posmap``, groundingdino/util/inference.py:48-79, util/utils.py:598-624).

As an op chain the tail is boolean-mask indexing -- ``sigmoid -> max(dim) -> > box_threshold -> prob[mask], boxes[mask] ->
> text_threshold -> nonzero per row`` -- every masked index a device-to-host synchronisation and an allocation whose size depends
on the data, none of it capturable.  ``ground`` is the same selection as ONE launch for the batch (csrc/grounding.hip) with
fixed-size padded outputs and a count per image, bit-identical to the chain; ``ground_reference`` is the chain itself, with the
same outputs and padding, for CPU tensors and the shapes the kernel declines.  ``predict`` is the reference's ``predict`` for a
batch on top of ``GroundingDINO.forward_grounding``: one call to ``ground``, one host read."""
from collections import namedtuple

import torch

from . import _lib

MAX_B, MAX_Q, MAX_T = 65535, 1024, 256
_WS = {}

# query [B, Q] int32, score [B, Q] fp32, box [B, Q, 4] fp32 (cxcywh, as given), argmax_token [B, Q] int32,
# token_bits [B, Q, ceil(T / 32)] int32 (the bit patterns of uint32 words: bit t % 32 of word t / 32), n_keep [B] int32;
# the first n_keep[b] positions of image b are the kept queries, everything behind them is zero
Grounded = namedtuple("Grounded", "query score box argmax_token token_bits n_keep")


def _limits(B, Q, T) -> bool:
    return 1 <= B <= MAX_B and 1 <= Q <= MAX_Q and 1 <= T <= MAX_T


def supported(prob, boxes) -> bool:
    """True where ``ground`` runs the kernel; everything else takes the chain that defines it."""
    return (torch.is_tensor(prob) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() == 3
            and torch.is_tensor(boxes) and boxes.device == prob.device and boxes.dtype == torch.float32
            and tuple(boxes.shape) == tuple(prob.shape[:2]) + (4,) and _limits(*prob.shape))


def _workspace(dev, nbytes):
    """The entry's workspace, cached per (device, stream) like ``topk._workspace``; inside a capture it comes from the graph's pool."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _check(prob, boxes, order):
    if not (torch.is_tensor(prob) and prob.dim() == 3 and prob.dtype == torch.float32 and torch.is_tensor(boxes)
            and boxes.dtype == torch.float32 and tuple(boxes.shape) == tuple(prob.shape[:2]) + (4,)):
        raise ValueError("ground: prob [B, Q, T] and boxes [B, Q, 4], both fp32")
    if order not in (0, 1):
        raise ValueError("ground: order is 0 (ascending query) or 1 (descending score)")


def ground_reference(prob, boxes, box_threshold, text_threshold, order=0):
    """The definition, as torch ops on the tensors' own device: per image ``s = prob.max(dim=1)``, ``mask = s > box_threshold``,
    the masked rows in ascending query order (``order = 0``) or in the stable descending order of their scores (``order = 1``),
    and per kept row the bits of ``row > text_threshold``.  Both thresholds are rounded to fp32 first, as the kernel receives
    them."""
    _check(prob, boxes, order)
    B, Q, T = prob.shape
    W = (T + 31) // 32
    dev = prob.device
    box_thr = torch.tensor(float(box_threshold), dtype=torch.float32, device=dev)
    text_thr = torch.tensor(float(text_threshold), dtype=torch.float32, device=dev)
    score, arg = prob.max(dim=2)                                  # a NaN in a row makes its score NaN
    mask = score > box_thr                                        # ... which no threshold is below
    hits = torch.zeros((B, Q, W * 32), dtype=torch.bool, device=dev)
    hits[..., :T] = prob > text_thr
    weights = torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev)
    words = (hits.view(B, Q, W, 32).to(torch.int64) * weights).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)   # the uint32 word's bit pattern
    out = Grounded(torch.zeros((B, Q), dtype=torch.int32, device=dev), torch.zeros((B, Q), dtype=torch.float32, device=dev),
                   torch.zeros((B, Q, 4), dtype=torch.float32, device=dev), torch.zeros((B, Q), dtype=torch.int32, device=dev),
                   torch.zeros((B, Q, W), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
    for b in range(B):
        idx = mask[b].nonzero().flatten()
        if order == 1:
            idx = idx[torch.sort(score[b][idx], descending=True, stable=True).indices]
        n = int(idx.numel())
        out.query[b, :n] = idx.to(torch.int32)
        out.score[b, :n] = score[b][idx]
        out.box[b, :n] = boxes[b][idx]
        out.argmax_token[b, :n] = arg[b][idx].to(torch.int32)
        out.token_bits[b, :n] = words[b][idx]
        out.n_keep[b] = n
    return out


def ground(prob, boxes, box_threshold, text_threshold, order=0):
    """prob [B, Q, T] (probabilities), boxes [B, Q, 4] -> ``Grounded``: one launch on the current stream, no host
    synchronisation, capturable.  Inputs the kernel does not serve (``supported``) take ``ground_reference``."""
    _check(prob, boxes, order)
    if not supported(prob, boxes):
        return ground_reference(prob, boxes, box_threshold, text_threshold, order)
    prob, boxes = prob.detach().contiguous(), boxes.detach().contiguous()
    B, Q, T = prob.shape
    W = (T + 31) // 32
    lib = _lib.load()
    nbytes = lib.zira_ground_workspace_bytes(B, Q, T)
    if nbytes == 0:
        raise RuntimeError("zira_ground_f32 does not serve B=%d Q=%d T=%d" % (B, Q, T))
    dev = prob.device
    out = Grounded(torch.empty((B, Q), dtype=torch.int32, device=dev), torch.empty((B, Q), dtype=torch.float32, device=dev),
                   torch.empty((B, Q, 4), dtype=torch.float32, device=dev), torch.empty((B, Q), dtype=torch.int32, device=dev),
                   torch.empty((B, Q, W), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        ws = _workspace(dev, nbytes)
        rc = lib.zira_ground_f32(prob.data_ptr(), boxes.data_ptr(), B, Q, T, float(box_threshold), float(text_threshold),
                                 int(order), out.query.data_ptr(), out.score.data_ptr(), out.box.data_ptr(),
                                 out.argmax_token.data_ptr(), out.token_bits.data_ptr(), out.n_keep.data_ptr(),
                                 ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("zira_ground_f32 failed: hipError %d" % rc)
    return out


# ---- the host side of the tail: strings -----------------------------------------------------------------------------------
def preprocess_caption(caption: str) -> str:
    """Lower-case, stripped, with a trailing "." (reference inference.py:17-21)."""
    result = caption.lower().strip()
    return result if result.endswith(".") else result + "."


class WordTable:
    """A tokenization of ONE caption reduced to what the phrase decoding reads: ``token_to_word(i)`` -> the index of the word
    token i belongs to, or None for a token that belongs to none ([CLS], [SEP], padding, positions behind the end)."""

    def __init__(self, table):
        self.table = list(table)

    def token_to_word(self, i):
        return self.table[i] if 0 <= i < len(self.table) else None


def tokenize_caption(tokenizer, caption):
    """-> an object with ``token_to_word`` for one caption.  A tokenizer whose output knows its words (transformers' fast
    tokenizers) is asked; ``bert.SimpleTokenizer`` makes one token per word between [CLS] and [SEP], so its table is the count of
    the word tokens in front, read off the ids it returns."""
    tok = tokenizer([caption], padding="longest", return_tensors="pt")
    if callable(getattr(tok, "token_to_word", None)):
        n = int(tok["input_ids"].shape[1])
        return WordTable([tok.token_to_word(0, i) for i in range(n)])
    special = {getattr(tokenizer, name) for name in ("cls_id", "sep_id", "pad_id") if hasattr(tokenizer, name)}
    if not special:
        raise TypeError("tokenize_caption: the tokenizer's output has no token_to_word and the tokenizer names no special ids")
    table, words = [], 0
    for tid, live in zip(tok["input_ids"][0].tolist(), tok["attention_mask"][0].tolist()):
        if not live or tid in special:
            table.append(None)
        else:
            table.append(words)
            words += 1
    return WordTable(table)


def _set_bits(token_bits_row):
    row = token_bits_row.tolist() if hasattr(token_bits_row, "tolist") else list(token_bits_row)
    return [32 * w + j for w, word in enumerate(row) for j in range(32) if (int(word) >> j) & 1]


def phrases_from_bits(token_bits_row, tokenized, caption: str) -> str:
    """The string of the reference's ``get_phrases_from_posmap(prob_row > text_threshold, tokenized, caption).replace(".", "")``
    from the row's mask words: the set tokens' word indices (tokens without a word skipped) select, in order, among the pieces
    of ``caption.split(".")``, which are joined by a blank."""
    used = set()
    for t in _set_bits(token_bits_row):
        word = tokenized.token_to_word(t)
        if word is not None:
            used.add(word)
    pieces = [piece for i, piece in enumerate(caption.split(".")) if i in used]
    return " ".join(pieces).replace(".", "")


def phrase_labels(token_bits):
    """token_bits [B, Q, W] -> [B, Q] int64: the first row of the image with the same mask words.  Rows of one label decode
    to one phrase."""
    same = (token_bits[:, :, None, :] == token_bits[:, None, :, :]).all(dim=-1)
    return same.to(torch.uint8).argmax(dim=-1)


def predict(model, batched_inputs, box_threshold, text_threshold, order=0, nms_threshold=None, nms_per_phrase=False):
    """The reference's ``predict`` for a batch: every input carries its image and its own ``"captions"`` string.  Per image
    ``(boxes [n, 4] cxcywh in 0..1, logits [n], phrases)`` on the host.  The model runs in eval mode without gradients; the
    selection is one ``ground`` launch (``Switches.native_grounding``; its twin otherwise) and one host read: the counts, then
    the kept slices.

    ``nms_threshold``: box NMS (nms.py) of the kept rows at this IoU, one more launch in front of the same host read (now of
    the counts behind the suppression) -- among all rows of an image, or with ``nms_per_phrase`` only among the rows whose token
    masks are the same (``phrase_labels``).  The survivors come back in the tail's own order."""
    from . import nms
    from .box_ops import box_cxcywh_to_xyxy
    from .transformer import Switches

    inputs = [dict(x, captions=preprocess_caption(x["captions"])) for x in batched_inputs]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model.forward_grounding(inputs)
            prob = out["pred_logits"].sigmoid()
            run = ground if Switches.native_grounding else ground_reference
            g = run(prob, out["pred_boxes"], box_threshold, text_threshold, order)
            captions = model._captions(inputs)[0]           # (what the text encoder saw: eval may append learned names)
            if nms_threshold is not None:
                labels = phrase_labels(g.token_bits) if nms_per_phrase else None
                keep, n_nms = nms.nms_padded(box_cxcywh_to_xyxy(g.box), g.score, labels, g.n_keep, nms_threshold)
    finally:
        model.train(was_training)
    if nms_threshold is None:
        rows = [slice(0, n) for n in g.n_keep.tolist()]
    else:
        rows = [keep[b, :n].to(torch.int64).sort().values for b, n in enumerate(n_nms.tolist())]
    results = []
    for b, sel in enumerate(rows):
        tokenized = tokenize_caption(model.tokenizer, captions[b])
        bits = g.token_bits[b, sel].cpu()
        results.append((g.box[b, sel].cpu(), g.score[b, sel].cpu(),
                        [phrases_from_bits(row, tokenized, captions[b]) for row in bits.tolist()]))
    return results
