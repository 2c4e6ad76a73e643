"""csrc/topk.hip through ``topk.topk_rows`` on the GPU against its definition -- the first k of
``torch.sort(stable=True, descending=True)`` computed on the CPU copy of the same tensor -- with ``torch.equal`` on the indices
and on the values' bit patterns (the definition is total: nothing is masked or skipped); against ``torch.topk`` where no two
values tie; repeatability; capture into a hipGraph and replay on fresh inputs; and the two-stage query selection with
``Switches.native_topk`` beside the parent's paths, eagerly and inside the decoder's graph."""
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from seeded import fill_by_name_  # noqa: E402

from ziragroundingdino_amd import graphs as zg  # noqa: E402
from ziragroundingdino_amd import topk, transformer, utils  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [(2, 22223, 900), (2, 6300, 300)]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(x_cpu, k):
    x = x_cpu.cuda()
    assert topk.supported(x, k)
    val, idx = topk.topk_rows(x, k)
    want_val, want_idx = torch.sort(x_cpu, dim=1, descending=True, stable=True)
    want_val, want_idx = want_val[:, :k], want_idx[:, :k]
    assert idx.dtype == torch.int64 and val.dtype == torch.float32 and tuple(idx.shape) == (x.shape[0], k)
    assert torch.equal(idx.cpu(), want_idx)
    assert torch.equal(_bits(val.cpu()), _bits(want_val))
    return val, idx


@pytest.mark.parametrize("rows,n,k", MODEL_SHAPES + [(2, 230400, 300), (1, 1024, 1024), (7, 5000, 1), (3, 777, 777),
                                                     (2, 40000, 1000), (5, 63, 5), (2, 32768, 64), (2, 32769, 64)])
def test_random_rows_match_the_definition(rows, n, k):
    g = torch.Generator().manual_seed(rows * 1000 + k)
    _check(torch.randn(rows, n, generator=g), k)


@pytest.mark.parametrize("rows,n,k", MODEL_SHAPES + [(2, 230400, 300)])
def test_heavy_ties_match_the_definition(rows, n, k):
    g = torch.Generator().manual_seed(n)
    levels = torch.randn(16, generator=g)
    _check(levels[torch.randint(0, 16, (rows, n), generator=g)], k)       # the k-th value is tied hundreds of times over


@pytest.mark.parametrize("rows,n,k", MODEL_SHAPES + [(2, 230400, 300)])
def test_special_values_match_the_definition(rows, n, k):
    g = torch.Generator().manual_seed(k)
    _check(torch.full((rows, n), -100.0), k)                              # recover_to_cls_logits' fill value everywhere
    x = torch.zeros(rows, n)
    x[torch.rand(rows, n, generator=g) < 0.5] = -0.0                      # +-0.0 mixed: one value
    x[:, ::97] = -1.0
    x[:, 5::1013] = 1.0
    _check(x, k)
    x = torch.randn(rows, n, generator=g)
    x[0, 17] = x[0, n - 1] = x[rows - 1, n // 2] = float("nan")           # NaN in three places: in front, by index
    x[0, 3] = float("inf")
    x[rows - 1, 4] = float("-inf")
    val, idx = _check(x, k)
    assert idx[0, :3].tolist() == [17, n - 1, 3]
    mag = torch.randint(0, 1 << 23, (rows, n), generator=g, dtype=torch.int32).view(torch.float32)   # denormals (and a few zeros)
    sign = torch.where(torch.rand(rows, n, generator=g) < 0.5, -1.0, 1.0)
    x = mag * sign
    assert float(x.abs().max()) < 1.2e-38 and int((x != 0).sum()) > rows * n // 2
    _check(x, k)


@pytest.mark.parametrize("rows,n,k", MODEL_SHAPES)
def test_equals_torch_topk_where_nothing_ties(rows, n, k):
    g = torch.Generator().manual_seed(n + k)
    x = torch.stack([torch.randperm(n, generator=g).float() for _ in range(rows)]) * 0.37 - 123.0   # n < 2^24: all distinct
    assert all(int(torch.unique(r).numel()) == n for r in x)
    val, idx = _check(x, k)
    want = torch.topk(x.cuda(), k, dim=1)
    assert torch.equal(idx, want.indices) and torch.equal(_bits(val), _bits(want.values))


def test_four_calls_on_tied_input_are_identical():
    g = torch.Generator().manual_seed(5)
    levels = torch.randn(16, generator=g)
    x = levels[torch.randint(0, 16, (2, 22223), generator=g)].cuda()
    first = topk.topk_rows(x, 900)
    for _ in range(3):
        again = topk.topk_rows(x, 900)
        assert torch.equal(again[1], first[1]) and torch.equal(_bits(again[0]), _bits(first[0]))


@pytest.mark.parametrize("rows,n,k", MODEL_SHAPES)
def test_captured_entry_replays_on_fresh_inputs(rows, n, k):
    """The entry inside ``torch.cuda.graph`` (this package's kernel and the copies around it, one branch), replayed three
    times with the static input overwritten by a different tensor each time."""
    g = torch.Generator().manual_seed(k)
    static = torch.randn(rows, n, generator=g).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            topk.topk_rows(static, k)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        val, idx = topk.topk_rows(static, k)
    levels = torch.randn(16, generator=g)
    fresh = [torch.randn(rows, n, generator=g), levels[torch.randint(0, 16, (rows, n), generator=g)],
             torch.randn(rows, n, generator=g) * 1e-3]
    for x in fresh:
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        want_val, want_idx = torch.sort(x, dim=1, descending=True, stable=True)
        assert torch.equal(idx.cpu(), want_idx[:, :k])
        assert torch.equal(_bits(val.cpu()), _bits(want_val[:, :k]))


# ---- consumer A: two-stage query selection ------------------------------------------------------------------------------
def _tiny_transformer():
    g = torch.load(os.path.join(GOLDEN, "mod_tiny_transformer.pt"), weights_only=False)
    kw = g["kwargs"]
    d = kw["d_model"]
    tr = transformer.Transformer(**kw)
    bbox = utils.MLP(d, d, 4, 3)
    cls = utils.ContrastiveEmbed(max_text_len=16)
    tr.decoder.bbox_embed = torch.nn.ModuleList([bbox for _ in range(2)])
    tr.decoder.class_embed = torch.nn.ModuleList([cls for _ in range(2)])
    tr.enc_out_bbox_embed = utils.MLP(d, d, 4, 3)
    tr.enc_out_class_embed = cls
    fill_by_name_(tr, g["salt"], g["scale"], g["scales"])
    tr.cuda().eval()
    g = {k: ([t.cuda() for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else v.cuda() if torch.is_tensor(v) else v)
         for k, v in g.items()}
    return tr, g


def _text_dict(g, text):
    return {"encoded_text": text, "text_token_mask": g["text_token_mask"], "position_ids": g["position_ids"],
            "text_self_attention_masks": g["text_self_attention_masks"]}


def test_selection_with_native_topk_equals_the_parent_paths(monkeypatch):
    tr, g = _tiny_transformer()
    seen = []
    real = topk.topk_rows

    def spy(x, k):
        seen.append(x.detach().clone())
        return real(x, k)

    monkeypatch.setattr(topk, "topk_rows", spy)

    def run(native):
        monkeypatch.setattr(transformer.Switches, "native_topk", native)
        srcs = [s.clone().requires_grad_(True) for s in g["srcs"]]
        text = g["text"].clone().requires_grad_(True)
        hs, refs, hs_enc, ref_enc, init_box, _ = tr(srcs, g["masks"], None, g["poss"], None, None, _text_dict(g, text))
        total = sum((h * go).sum() for h, go in zip(hs, g["grad_hs"])) + (refs[-1] ** 2).sum() + (hs_enc ** 2).sum() * 0.1
        grads = torch.autograd.grad(total, srcs)
        return tr.last_topk_proposals.clone(), hs, refs, grads

    idx_n, hs_n, refs_n, grads_n = run(True)
    assert len(seen) == 1                                  # the kernel served the selection
    logits, k = seen[0], tr.num_queries
    top = torch.sort(logits, dim=1, descending=True)[0][:, :k + 1]
    assert bool((top[:, :-1] > top[:, 1:]).all())          # nothing ties down to the (k+1)-th logit: torch.topk is determined
    idx_p, hs_p, refs_p, grads_p = run(False)
    assert len(seen) == 1
    assert torch.equal(idx_n, idx_p) and torch.equal(idx_n, g["topk_proposals"])
    for a, b in zip(list(hs_n) + list(refs_n) + list(grads_n), list(hs_p) + list(refs_p) + list(grads_p)):
        assert torch.equal(_bits(a), _bits(b))


def test_graphed_selection_picks_what_the_eager_path_picks(monkeypatch):
    """``_SelectDecodePiece`` (selection inside the decoder's graph) and the eager path run the same kernel with the switch
    on: the same proposals, which the stable-sort stand-in could not promise under ties."""
    from test_model_gpu import small_model
    from ziragroundingdino_amd.train import synthetic_batch

    monkeypatch.setattr(transformer.Switches, "native_topk", True)
    monkeypatch.setattr(zg.GraphedTransformer, "graph_selection", True)
    calls = []
    real = topk.topk_rows
    monkeypatch.setattr(topk, "topk_rows", lambda x, k: (calls.append(torch.cuda.is_current_stream_capturing()), real(x, k))[1])
    model = small_model().train()       # the product's route into the graphs: a frozen transformer in a training forward
    model.before_train()
    data = synthetic_batch(2, 224, 320, n_categories=4, boxes_per_image=3, device="cuda")
    model.use_transformer_graph = False
    model(data)
    torch.cuda.synchronize()
    eager = model.transformer.last_topk_proposals.clone()
    assert calls == [False]
    model.use_transformer_graph = True
    for _ in range(2):                                     # the first call captures, the second replays
        model(data)
        torch.cuda.synchronize()
        assert torch.equal(model.transformer.last_topk_proposals, eager)
    assert any(calls[1:]), "the selection was not captured into the decoder's graph"
