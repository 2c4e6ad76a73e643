"""Chunked vocabularies without a GPU: the C ABI of the merged tail is declared in include/zira_vocab.h, typed from that header
into tables of its own and exported by the built library; argument errors are answered on the host; ``split_categories`` on the
tokenizer stub; ``detections_chunked_reference`` on hand-worked cases, against the brute-force virtual row and against the
op-chain tail; and the slice model: untouched with the switch at its default, identical for a one-chunk list, equal to the
manual per-chunk loop for a list forced into three chunks."""
import ctypes
import os
import re
import types

import pytest
import torch

from conftest import GOLDEN, ROOT
from test_train_step import build_slice_model, slice_inputs

from ziragroundingdino_amd import _lib
from ziragroundingdino_amd import bert as zbert
from ziragroundingdino_amd import build as zbuild
from ziragroundingdino_amd import topk, vocab
from ziragroundingdino_amd.bert import SimpleTokenizer
from ziragroundingdino_amd.box_ops import box_cxcywh_to_xyxy
from ziragroundingdino_amd.groundingdino import GroundingDINO
from ziragroundingdino_amd.structures import Boxes, Instances, detector_postprocess

ENTRIES = ["zira_det_merge_lds_bytes", "zira_det_merge_f32"]
EINVAL = 1
STATIC_LDS = 1024 * 8 + 256 * 8 * 4 + 2 * 16 * 4 + 8 + 3 * 64 * 4      # the selection's state and the chunk table


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_typed_and_exported():
    text = open(os.path.join(ROOT, "include", "zira_vocab.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)
    assert declared == ENTRIES == list(_lib.VOCAB_SYMBOLS) == list(_lib.VOCAB_PROTOTYPES)
    zbuild.build_extension()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ENTRIES:
        assert hasattr(raw, sym), "libzira_msda.so does not export %s" % sym
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    P = _lib.VOCAB_PROTOTYPES
    S = _lib.VOCAB_STRUCTS["zira_vocab_chunks"]
    assert P["zira_det_merge_lds_bytes"] == (sz, [i])
    assert P["zira_det_merge_f32"] == (i, [vp, vp, ctypes.POINTER(S), vp, i, i, i, vp, vp, vp, vp, vp, vp])
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert _lib.VOCAB_CONSTANTS == {"ZIRA_VOCAB_MAX_CHUNKS": 64, "ZIRA_VOCAB_MAX_CANDIDATES": 16384, "ZIRA_VOCAB_MAX_K": 1024,
                                    "ZIRA_VOCAB_MAX_B": 65535}
    assert list(_lib.VOCAB_STRUCTS) == ["zira_vocab_chunks"] and _lib.VocabChunks is S and ctypes.sizeof(S) == 8 + 3 * 64 * 4
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("J", 0), ("n", 4), ("start", 8), ("classes", 264),
                                                                   ("label_offset", 520)]
    assert (vocab.MAX_CHUNKS, vocab.MAX_CANDIDATES, vocab.MAX_K, vocab.MAX_B) == (64, 16384, 1024, 65535)


def test_the_first_header_s_surface_is_what_it_was():
    assert len(_lib.SYMBOLS) == 100 and not set(ENTRIES) & set(_lib.SYMBOLS)
    assert not any("VOCAB" in name for name in _lib.CONSTANTS) and "zira_vocab_chunks" not in _lib.STRUCTS
    assert len(_lib.NMS_SYMBOLS) == 2 and list(_lib.METRICS_STRUCTS) == ["zira_metrics_sources"]
    assert os.path.join(ROOT, "include", "zira_vocab.h") in [os.path.normpath(h) for h in zbuild.HEADERS]
    assert "vocab.hip" in [os.path.basename(s) for s in zbuild.SOURCES]
    # the box arithmetic's flags: topk.hip has none of its own (intrinsics under `fp contract(off)`); vocab.hip says it again
    assert "topk.hip" not in zbuild.EXTRA_FLAGS and zbuild.EXTRA_FLAGS["vocab.hip"] == ["-ffp-contract=off"]


def _chunks(J=2, n=600, start=(0, 300), classes=(7, 3), offset=(0, 7)):
    c = _lib.VocabChunks()
    c.J, c.n = J, n
    for j, (s, k, o) in enumerate(zip(start, classes, offset)):
        c.start[j], c.classes[j], c.label_offset[j] = s, k, o
    return c


def test_argument_errors_are_answered_on_the_host():
    """Nothing is launched: there is no device here, and the host pointers are never looked at."""
    lib = _lib.load()

    def call(B=2, Q=900, k=300, chunks=None, **ptr):
        p = dict(cand_scores=64, cand_index=64, boxes=64, sizes=64, scores=64, labels=64, xyxy=64, n_keep=64)
        p.update(ptr)
        c = _chunks() if chunks is None else chunks
        return lib.zira_det_merge_f32(p["cand_scores"], p["cand_index"], None if c == "null" else ctypes.byref(c), p["boxes"],
                                      B, Q, k, p["sizes"], p["scores"], p["labels"], p["xyxy"], p["n_keep"], None)

    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(Q=0), dict(k=0), dict(k=1025), dict(k=-3), dict(chunks="null"),
                dict(Q=1 << 30)):                                                     # (Q * C_j past 2^31)
        assert call(**bad) == EINVAL, bad
    for null in ("cand_scores", "cand_index", "boxes", "sizes", "scores", "labels", "xyxy", "n_keep"):
        assert call(**{null: None}) == EINVAL, null
    for name, ptr in (("boxes", 72), ("xyxy", 72), ("cand_index", 68), ("labels", 68), ("cand_scores", 66), ("sizes", 66),
                      ("scores", 66), ("n_keep", 66)):
        assert call(**{name: ptr}) == EINVAL, name
    for table in (_chunks(J=0), _chunks(J=65), _chunks(n=0), _chunks(n=16385), _chunks(start=(1, 300)), _chunks(start=(0, 0)),
                  _chunks(start=(0, 600)), _chunks(start=(0, 700)), _chunks(classes=(7, 0)), _chunks(offset=(0, -1)),
                  _chunks(J=3, start=(0, 300, 200), classes=(7, 3, 1), offset=(0, 7, 10)),
                  _chunks(offset=(0, 2 ** 31 - 2))):
        assert call(chunks=table) == EINVAL, (table.J, table.n, list(table.start[:3]))
    # the LDS the launch takes: a key per candidate position beside the static state
    assert lib.zira_det_merge_lds_bytes(1) == 4 + STATIC_LDS == 17292
    assert lib.zira_det_merge_lds_bytes(16384) == 16384 * 4 + STATIC_LDS <= 160 * 1024
    assert lib.zira_det_merge_lds_bytes(0) == lib.zira_det_merge_lds_bytes(16385) == lib.zira_det_merge_lds_bytes(-3) == 0


# ---- split_categories ------------------------------------------------------------------------------------------------------------
NAMES = ["fish", "jellyfish", "penguin", "puffin", "shark", "starfish", "stingray", "crab", "turtle", "seal", "whale"]


def test_split_categories():
    tok = SimpleTokenizer()
    count = lambda chunk: vocab.caption_tokens(vocab.caption_of(chunk), tok)
    assert count(NAMES[:4]) == 2 + 2 * 4                                  # [CLS] + (word, ".") per name + [SEP]
    assert vocab.split_categories(NAMES, tok, 256) == [NAMES]             # a list that fits: one chunk
    assert vocab.split_categories(NAMES, tok, 2 + 2 * len(NAMES)) == [NAMES]      # ... exactly
    got = vocab.split_categories(NAMES, tok, 10)                          # four names are 10 tokens: the boundary falls on the limit
    assert got == [NAMES[0:4], NAMES[4:8], NAMES[8:11]] and all(count(c) <= 10 for c in got) and count(NAMES[:5]) > 10
    assert vocab.split_categories(NAMES, tok, 11) == got                  # one token more buys nothing
    assert vocab.split_categories(NAMES, tok, 256, chunk_size=3) == [NAMES[0:3], NAMES[3:6], NAMES[6:9], NAMES[9:11]]
    assert vocab.split_categories(NAMES, tok, 10, chunk_size=5) == got    # both caps: the tighter one rules
    assert vocab.split_categories(NAMES, tok, 256, chunk_size=1) == [[n] for n in NAMES]
    long = ["sea lion", "a very long name of eleven words that does not fit at all", "eel"]
    mixed = vocab.split_categories(["sea lion", "great white shark", "eel", "crab"], tok, 8)     # names of 2, 3, 1, 1 words
    assert mixed == [["sea lion"], ["great white shark", "eel"], ["crab"]]    # 5; 4 + 2 + 2 = 8; 4 tokens
    for chunks, names in ((got, NAMES), (mixed, ["sea lion", "great white shark", "eel", "crab"])):
        assert [n for c in chunks for n in c] == names                    # order kept, nothing lost
    with pytest.raises(ValueError, match="a very long name of eleven words"):
        vocab.split_categories(long, tok, 10)
    with pytest.raises(ValueError):
        vocab.split_categories(NAMES, tok, 10, chunk_size=0)
    assert vocab.split_categories([], tok, 10) == []


# ---- the definition ------------------------------------------------------------------------------------------------------------
def candidates(probs, k, extra=0):
    """The caller's side of the scheme: per chunk ``topk_rows`` of its [B, Q * C_j] into its slice of the candidate row
    (``extra`` positions of padding behind every chunk's candidates, left as garbage for ``merge_detections`` to define)."""
    B = probs[0].shape[0]
    widths = [min(k, p.shape[1] * p.shape[2]) for p in probs]
    start = [0]
    for w in widths:
        start.append(start[-1] + w + extra)
    cand_scores = torch.full((B, start[-1]), 7.0, dtype=probs[0].dtype, device=probs[0].device)      # above every probability
    cand_index = torch.full((B, start[-1]), 10 ** 9, dtype=torch.int64, device=probs[0].device)
    for j, (p, w) in enumerate(zip(probs, widths)):
        val, idx = topk.topk_rows(p.reshape(B, -1), w)
        cand_scores[:, start[j]:start[j] + w], cand_index[:, start[j]:start[j] + w] = val, idx
    classes = [p.shape[2] for p in probs]
    offset = [sum(classes[:j]) for j in range(len(classes))]
    return cand_scores, cand_index, start, classes, offset


def op_chain_tail(top, label, picked, k, sizes):
    """dt_inference's boxes + detector_postprocess per image, padded as the tails pad."""
    B = top.shape[0]
    out = (torch.zeros(B, k, dtype=top.dtype), torch.zeros(B, k, dtype=torch.int64), torch.zeros(B, k, 4, dtype=picked.dtype),
           torch.zeros(B, dtype=torch.int32))
    for b, (ih, iw, oh, ow) in enumerate(sizes.tolist()):
        r = Instances((ih, iw), pred_boxes=Boxes(box_cxcywh_to_xyxy(picked[b])), scores=top[b], pred_classes=label[b])
        r.pred_boxes.scale(scale_x=iw, scale_y=ih)
        r = detector_postprocess(r, oh, ow)
        n = len(r)
        out[0][b, :n], out[1][b, :n], out[2][b, :n], out[3][b] = r.scores, r.pred_classes, r.pred_boxes.tensor, n
    return out


def brute_force(probs, boxes, k, sizes):
    """The first k of a stable descending sort of the virtual row cat_j(prob_j[b].flatten()), boxes gathered per chunk."""
    B, Q = probs[0].shape[:2]
    virtual = torch.cat([p.reshape(B, -1) for p in probs], dim=1)
    val, pos = torch.sort(virtual, dim=1, descending=True, stable=True)
    val, pos = val[:, :k], pos[:, :k]
    label = torch.zeros_like(pos)
    picked = torch.zeros(B, pos.shape[1], 4, dtype=boxes.dtype)
    for b in range(B):
        for r, p in enumerate(pos[b].tolist()):
            j, seen = 0, 0
            while p >= Q * probs[j].shape[2]:
                p -= Q * probs[j].shape[2]
                seen += probs[j].shape[2]
                j += 1
            C = probs[j].shape[2]
            label[b, r], picked[b, r] = seen + p % C, boxes[j, b, p // C]
    return op_chain_tail(val, label, picked, k, sizes)


def assert_same(got, want, what=""):
    names = ("scores", "labels", "xyxy", "n_keep")
    for name, a, b in zip(names, got, want):
        a, b = a.cpu(), b.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.is_floating_point():
            a, b = a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)
        assert torch.equal(a, b), (what, name)
    assert got[1].dtype == torch.int64 and got[3].dtype == torch.int32


SIZES1 = torch.tensor([[100.0, 200.0, 100.0, 200.0]])
BOX = [0.5, 0.5, 0.25, 0.25]                  # -> (75, 37.5, 125, 62.5) in a 100 x 200 image: exact in fp32


def _hand(scores, index, start, classes, offset, boxes, k, sizes=SIZES1):
    out = vocab.detections_chunked_reference(torch.tensor([scores]), torch.tensor([index]), start, classes, offset,
                                             torch.tensor(boxes)[:, None], k, sizes)
    n = int(out[3][0])
    assert out[0].shape == (1, k) and out[2].shape == (1, k, 4) and out[1].dtype == torch.int64 and out[3].dtype == torch.int32
    assert not out[0][0, n:].any() and not out[1][0, n:].any() and not out[2][0, n:].any()
    return out[0][0, :n].tolist(), out[1][0, :n].tolist(), out[2][0, :n].tolist()


def test_reference_hand_worked_ties_and_labels():
    boxes = [[BOX, BOX], [BOX, BOX]]                                      # J = 2, Q = 2
    # chunk 0: C = 3 (labels 0..2), chunk 1: C = 2 (labels 3..4); a tie across the chunks goes to the lower chunk
    s, l, x = _hand([0.5, 0.25, 0.5, 0.125], [4, 0, 1, 2], [0, 2, 4], [3, 2], [0, 3], boxes, 2)
    assert s == [0.5, 0.5] and l == [0 + 4 % 3, 3 + 1 % 2] and x[0] == [75.0, 37.5, 125.0, 62.5]
    # a tie inside a chunk goes to the lower position (the chunk's own top-k put the lower index there)
    s, l, _ = _hand([0.5, 0.5, 0.75, 0.5], [1, 5, 0, 3], [0, 2, 4], [3, 2], [0, 3], boxes, 3)
    assert s == [0.75, 0.5, 0.5] and l == [3, 1, 2]
    # label offsets are the caller's: any numbering
    _, l, _ = _hand([0.5, 0.25], [5, 1], [0, 1, 2], [3, 2], [100, 40], boxes, 2)
    assert l == [100 + 2, 40 + 1]


def test_reference_drops_empty_boxes_and_compacts():
    gone, wide = [1.5, 0.5, 0.25, 0.25], [0.5, 0.5, 0.0, 0.25]               # clipped to nothing; no width
    boxes = [[BOX, gone, wide, [0.25, 0.5, 0.5, 1.0]]]                    # J = 1, Q = 4, C = 1
    s, l, x = _hand([0.875, 0.75, 0.625, 0.5], [1, 0, 2, 3], [0, 4], [1], [0], boxes, 4)
    assert s == [0.75, 0.5] and l == [0, 0] and x == [[75.0, 37.5, 125.0, 62.5], [0.0, 0.0, 100.0, 100.0]]
    s, _, _ = _hand([0.9, 0.8], [1, 2], [0, 2], [1], [0], boxes, 2)       # every box empty
    assert s == []
    # the output size: boxes scale by out / img, the quotient rounded to fp32 once
    s, l, x = _hand([0.9], [0], [0, 1], [1], [0], boxes, 1, torch.tensor([[100.0, 200.0, 50.0, 300.0]]))
    assert x == [[112.5, 18.75, 187.5, 31.25]]


def test_reference_k_beyond_the_candidates_and_a_short_chunk():
    boxes = [[BOX, BOX], [BOX, BOX]]
    # k larger than all candidates: all of them, in order, the rest zero
    s, l, _ = _hand([0.5, 0.25, 0.75], [0, 1, 1], [0, 2, 3], [1, 1], [0, 1], boxes, 8)
    assert s == [0.75, 0.5, 0.25] and l == [1, 0, 0]
    # a chunk with Q * C_j = 2 < k = 3: its slice is 3 wide, merge_detections defines the padding position, the k taken are real
    cs, ci = torch.tensor([[0.5, 0.25, 9.0, 0.75, 0.6875, 0.625]]), torch.tensor([[0, 1, 12345, 3, 0, 2]])
    got = vocab.merge_detections(cs, ci, [0, 3, 6], [1, 2], [0, 1], torch.tensor(boxes)[:, None], 3, SIZES1)
    assert cs[0, 2] == float("-inf") and ci[0, 2] == 0                   # in place
    assert got[0][0].tolist() == [0.75, 0.6875, 0.625] and got[1][0].tolist() == [1 + 1, 1 + 0, 1 + 0] and int(got[3][0]) == 3
    want = vocab.detections_chunked_reference(cs, ci, [0, 3, 6], [1, 2], [0, 1], torch.tensor(boxes)[:, None], 3, SIZES1)
    assert_same(got, want)
    with pytest.raises(ValueError):
        vocab.merge_detections(cs, ci, [0, 3, 3], [1, 2], [0, 1], torch.tensor(boxes)[:, None], 3, SIZES1)     # not ascending
    with pytest.raises(ValueError):
        vocab.merge_detections(cs, ci, [0, 3, 6], [1, 2], [0, 1], torch.tensor(boxes), 3, SIZES1)              # boxes [J, B, Q, 4]


def _random_boxes(g, J, B, Q):
    boxes = torch.rand(J, B, Q, 4, generator=g)
    boxes[..., 2:] *= 0.6
    boxes[:, :, ::7, 0] += 0.8                                            # leave the image on the right
    boxes[:, :, 2::5, 2] = 0.0                                            # no width
    return boxes


SIZES3 = torch.tensor([[800.0, 1333.0, 800.0, 1333.0], [640.0, 1066.0, 480.0, 799.0], [600.0, 900.0, 1200.0, 1800.0]])


@pytest.mark.parametrize("Q,classes,k", [(5, (3, 7, 1), 4), (5, (3, 7, 1), 64), (16, (7, 7, 3, 1), 20), (1, (1, 3), 2)])
def test_two_level_scheme_is_the_brute_force_virtual_row(Q, classes, k):
    g = torch.Generator().manual_seed(Q * 100 + k)
    B = 3
    probs = [torch.randint(0, 6, (B, Q, C), generator=g).float() / 8 for C in classes]       # many repeated scores
    boxes = _random_boxes(g, len(classes), B, Q)
    cand = candidates(probs, k)
    got = vocab.detections_chunked_reference(*cand, boxes, k, SIZES3)
    want = brute_force(probs, boxes, k, SIZES3)
    assert_same(got, want)
    if k <= sum(min(k, Q * C) for C in classes):      # (with k beyond the real candidates the padding positions are taken too)
        assert_same(vocab.merge_detections(*candidates(probs, k, extra=2), boxes, k, SIZES3), want, "with padding positions")
    if Q == 16:
        assert 0 < int(got[3].min()) and int(got[3].max()) < k                                # some kept, some dropped


def test_shared_boxes_and_no_ties_is_the_op_chain_tail_on_the_concatenation():
    g = torch.Generator().manual_seed(5)
    B, Q, classes, k = 3, 16, (7, 3, 5), 40
    n = Q * sum(classes)
    logits = torch.stack([torch.linspace(-4, 4, n)[torch.randperm(n, generator=g)] for _ in range(B)]).view(B, Q, sum(classes))
    assert all(int(torch.unique(r).numel()) == n for r in logits.sigmoid().view(B, -1))
    one = _random_boxes(g, 1, B, Q)[0]
    probs = [p.contiguous() for p in logits.sigmoid().split(list(classes), dim=2)]
    got = vocab.merge_detections(*candidates(probs, k), one[None].repeat(len(classes), 1, 1, 1), k, SIZES3)
    stub = types.SimpleNamespace(select_box_nums_for_evaluation=k)
    image_sizes = [(int(r[0]), int(r[1])) for r in SIZES3.tolist()]
    chain = GroundingDINO.dt_inference(stub, logits, one, image_sizes)                        # torch.topk as it is
    for b, (r, row) in enumerate(zip(chain, SIZES3.tolist())):
        r = detector_postprocess(r, int(row[2]), int(row[3]))
        m = int(got[3][b])
        assert m == len(r) and 0 < m < k
        assert torch.equal(got[0][b, :m], r.scores) and torch.equal(got[1][b, :m], r.pred_classes)
        assert torch.equal(got[2][b, :m], r.pred_boxes.tensor)


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a CPU tensor reached the library"))
    g = torch.Generator().manual_seed(1)
    probs = [torch.rand(1, 5, 3, generator=g), torch.rand(1, 5, 2, generator=g)]
    cand = candidates(probs, 4)
    assert not vocab.supported(*cand, _random_boxes(g, 2, 1, 5), 4, SIZES1)
    out = vocab.merge_detections(*cand, _random_boxes(g, 2, 1, 5), 4, SIZES1)
    assert out[0].shape == (1, 4)


# ---- the model -----------------------------------------------------------------------------------------------------------------
class _Front:
    """What ``forward`` needs of the frozen front end the slice model does not have: the golden feature maps behind
    ``run_backbone``, their padding mask as ``samples``, the image sizes."""

    def __init__(self, g, model, dev):
        inp, feats, poss, _, _, _ = slice_inputs(g, model, dev)
        self.feats, self.poss = feats, poss
        self.samples = types.SimpleNamespace(mask=inp["img_mask"], device=torch.device(dev), no_padding=False)
        self.images = types.SimpleNamespace(image_sizes=[(64, 80), (60, 72)])
        self.batch = lambda captions: [{"captions": c, "height": h, "width": w} for c, (h, w) in zip(captions, [(64, 80), (90, 108)])]


def chunk_model(dev, monkeypatch):
    """The slice model with a front end: its text encoder gets BERT's vocabulary size (the tokenizer stub's ids), the frozen
    backbone is the golden feature maps."""
    g = torch.load(os.path.join(GOLDEN, "eval_zira_slice.pt"), weights_only=False)
    model = build_slice_model(g, dev).eval()
    torch.manual_seed(3)
    model.bert = zbert.BertModel(zbert.BertConfig(vocab_size=30522, hidden_size=g["cfg"]["bert_hidden"], num_hidden_layers=1,
                                                  num_attention_heads=4, intermediate_size=32, hidden_dropout_prob=0.0,
                                                  attention_probs_dropout_prob=0.0)).to(dev).eval()
    for p in model.bert.parameters():
        p.requires_grad = False
    model.use_frontend_graphs = False
    model.select_box_nums_for_evaluation = 20
    front = _Front(g, model, dev)
    monkeypatch.setattr(model, "_canvas_batch", lambda inputs: (front.images, front.samples))
    monkeypatch.setattr(model, "_canvas_sizes", ((64, 80),), raising=False)
    monkeypatch.setattr(model, "run_backbone", lambda samples: (front.feats, front.poss))
    return model, front


SEVEN = ["fish", "jellyfish", "penguin", "puffin", "shark", "starfish", "stingray"]


def instances_equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = a["instances"], b["instances"]
        assert tuple(a.image_size) == tuple(b.image_size) and list(a.__dict__) == list(b.__dict__) and len(a) == len(b)
        assert a.scores.dtype == b.scores.dtype and a.pred_classes.dtype == b.pred_classes.dtype
        assert torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)


def manual_loop(model, front, batch, chunks, merge):
    """The chunked forward by hand: per chunk the text side, the transformer, the heads and the chunk's top-k, then ``merge``."""
    B, k = len(batch), model.select_box_nums_for_evaluation
    probs, boxes = [], []
    for chunk in chunks:
        text_dict, c2t, loss = model.encode_text([".".join(chunk) + "."] * B, front.samples.device)
        out = model.forward_features(front.feats, front.poss, front.samples.mask, text_dict, c2t, loss, None)
        probs.append(out["pred_logits"][..., :len(chunk)].sigmoid().contiguous())
        boxes.append(out["pred_boxes"])
    sizes = torch.tensor([[ih, iw, x["height"], x["width"]] for (ih, iw), x in zip(front.images.image_sizes, batch)],
                         dtype=torch.float32, device=probs[0].device)
    return merge(*candidates(probs, k), torch.stack(boxes), k, sizes), probs


def test_model_default_and_one_chunk_are_today_s_forward(monkeypatch):
    model, front = chunk_model("cpu", monkeypatch)
    assert GroundingDINO.category_chunk_size is None and "category_chunk_size" not in model.__dict__
    batch = front.batch([".".join(SEVEN[:3]) + "."] * 2)
    with torch.no_grad():
        monkeypatch.setattr(vocab, "split_categories", lambda *a, **k: pytest.fail("the switch is off"))
        monkeypatch.setattr(vocab, "merge_detections", lambda *a, **k: pytest.fail("the switch is off"))
        plain = model(batch)
        monkeypatch.undo()
        model, front = chunk_model("cpu", monkeypatch)                      # (undo took the front end's patches too)
        batch = front.batch([".".join(SEVEN[:3]) + "."] * 2)
        assert len(plain) == 2 and len(plain[0]["instances"]) > 0
        instances_equal(model(batch), plain)
        model.category_chunk_size = "auto"                                   # three names are 8 of the 16 tokens: one chunk
        monkeypatch.setattr(vocab, "merge_detections", lambda *a, **k: pytest.fail("one chunk takes today's path"))
        instances_equal(model(batch), plain)
        model.category_chunk_size = 3
        instances_equal(model(batch), plain)
        # training mode ignores the switch
        model.category_chunk_size = 1
        monkeypatch.setattr(model, "_category_chunks", lambda names: pytest.fail("training mode ignores the switch"))
        monkeypatch.setattr(model, "forward_features", lambda *a, **k: "losses")
        monkeypatch.setattr(model, "prepare_targets", lambda *a: None)
        assert model.train()([dict(x, instances=types.SimpleNamespace(to=lambda d: None)) for x in batch]) == "losses"


@pytest.mark.parametrize("nms_threshold", [None, 0.5])
def test_model_three_chunks_equal_the_manual_loop_with_the_reference_merge(monkeypatch, nms_threshold):
    model, front = chunk_model("cpu", monkeypatch)
    model.nms_threshold_for_evaluation = nms_threshold
    batch = front.batch([".".join(SEVEN) + "."] * 2)
    model.category_chunk_size = 3
    assert model._category_chunks([SEVEN, SEVEN]) == [SEVEN[0:3], SEVEN[3:6], SEVEN[6:7]]
    calls = []
    real = vocab.merge_detections
    monkeypatch.setattr(vocab, "merge_detections", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        got = model(batch)
        assert calls == [1]                                                  # one merge for the batch
        (scores, labels, xyxy, n_keep), probs = manual_loop(model, front, batch, [SEVEN[0:3], SEVEN[3:6], SEVEN[6:7]],
                                                            vocab.detections_chunked_reference)
    want = model._padded_instances(scores, labels, xyxy, n_keep, [(64, 80), (90, 108)])
    instances_equal(got, want)
    assert all(0 < len(r["instances"]) <= 20 for r in got)
    seen = torch.cat([r["instances"].pred_classes for r in got])
    assert int(seen.max()) <= 6 and int(seen.max()) >= 3                     # global labels, the later chunks' among them
    if nms_threshold is None:                                                # the scores are the virtual row's best
        virtual = torch.cat([p.reshape(2, -1) for p in probs], dim=1).sort(dim=1, descending=True).values
        assert all(torch.equal(r["instances"].scores, virtual[b, :20][:len(r["instances"])]) or int(n_keep[b]) < 20
                   for b, r in enumerate(got))
    # "auto" with a token budget that forces the split: 16 tokens hold seven one-word names exactly, so shrink the budget
    model.category_chunk_size = "auto"
    assert model._category_chunks([SEVEN, SEVEN]) == [SEVEN]
    model._text_cache.clear()
    monkeypatch.setattr(model, "max_text_len", 8)
    assert model._category_chunks([SEVEN, SEVEN]) == [SEVEN[0:3], SEVEN[3:6], SEVEN[6:7]]


def test_model_mismatched_category_lists_raise(monkeypatch):
    model, front = chunk_model("cpu", monkeypatch)
    model.category_chunk_size = 3
    with pytest.raises(ValueError, match="share one category list"):
        model(front.batch([".".join(SEVEN) + ".", ".".join(SEVEN[:6]) + "."]))
    model.category_chunk_size = "all"
    with pytest.raises(ValueError, match="category_chunk_size"):
        model(front.batch([".".join(SEVEN) + "."] * 2))
