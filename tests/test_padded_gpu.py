"""Padded minibatches through the fused encoder attention node and the masked panel GEMM.

- ``zira_gemm_f16x2_panel_masked_f32`` (csrc/gemm_f16x2_panel.hip): the row mask against the unmasked entry, bit for bit.
- ``encoder_layer.padded_applies`` and the padded node against the module composition (reference
  transformer_for_adapter.py:888-899 with ``key_padding_mask``; only the value is masked, ms_deform_attn.py:287-288).
- The decoder's batched value projections with the mask inside the node.
- A two-image batch of different sizes through the frozen small model, eager and with the transformer graphs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ziragroundingdino_amd import _lib  # noqa: E402
from ziragroundingdino_amd import gemm_bf16x3 as g3  # noqa: E402


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------

def _masks(M, dev):
    g = torch.Generator(device="cpu").manual_seed(M)
    runs = torch.zeros(M, dtype=torch.bool)
    for a, b in ((5, 70), (95, 161), (M - 45, M)):        # runs that start and end inside 32-row blocks and cover whole ones
        runs[max(a, 0):max(b, 0)] = True
    return {"none": None, "all": torch.ones(M, dtype=torch.bool, device=dev),
            "random": (torch.rand(M, generator=g) < 0.3).to(dev), "runs": runs.to(dev)}


def _call_masked(a, frags, N, K, epi, bias, aux, mask, out):
    lib = _lib.load()
    rm = None if mask is None else mask.to(torch.uint8).contiguous()
    rc = lib.zira_gemm_f16x2_panel_masked_f32(a.data_ptr(), None, frags.data_ptr(), a.shape[0], N, K, epi,
                                              None if bias is None else bias.data_ptr(), None if aux is None else aux.data_ptr(),
                                              None if rm is None else rm.data_ptr(), out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _call_plain(a, frags, N, K, epi, bias, aux, out):
    lib = _lib.load()
    rc = lib.zira_gemm_f16x2_panel_f32(a.data_ptr(), None, frags.data_ptr(), a.shape[0], N, K, epi,
                                       None if bias is None else bias.data_ptr(), None if aux is None else aux.data_ptr(),
                                       out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return out


@pytest.mark.parametrize("N,K", [(256, 256), (384, 256)])
@pytest.mark.parametrize("M", [44446, 1000, 31])
def test_masked_panel_abi(M, N, K):
    dev = torch.device("cuda")
    torch.manual_seed(M + N)
    w = torch.randn(N, K, device=dev) * 0.05
    frags = g3.split_frags_f16x2(w, False)
    bias = torch.randn(N, device=dev)
    aux = torch.randn(M, N, device=dev)
    a = torch.randn(M, K, device=dev)
    for name, mask in _masks(M, dev).items():
        a_in = a.clone()
        if mask is not None:
            a_in[mask] = float("nan")            # whatever a padded row holds must not reach C
            a_in[mask.nonzero().flatten()[::3], 7] = float("inf")
        keep = torch.ones(M, dtype=torch.bool, device=dev) if mask is None else ~mask
        want_b = _call_plain(a_in, frags, N, K, g3.EPI_BIAS, bias, None, torch.empty(M, N, device=dev))
        want_a = _call_plain(a_in, frags, N, K, g3.EPI_ADD, None, aux, torch.empty(M, N, device=dev))
        # EPI_BIAS
        got = torch.full((M, N), 3.0, device=dev)
        assert _call_masked(a_in, frags, N, K, g3.EPI_BIAS, bias, None, mask, got) == 0
        assert torch.equal(got[keep], want_b[keep]), name
        if mask is not None:
            assert torch.equal(got[mask], torch.zeros_like(got[mask])), name
        # EPI_ADD out of place
        got = torch.full((M, N), 3.0, device=dev)
        assert _call_masked(a_in, frags, N, K, g3.EPI_ADD, None, aux, mask, got) == 0
        assert torch.equal(got[keep], want_a[keep]), name
        if mask is not None:
            assert torch.equal(got[mask], aux[mask]), name
        # EPI_ADD in place
        acc = aux.clone()
        assert _call_masked(a_in, frags, N, K, g3.EPI_ADD, None, acc, mask, acc) == 0
        assert torch.equal(acc[keep], want_a[keep]), name
        if mask is not None:
            assert torch.equal(acc[mask], aux[mask]), name
        assert not torch.isnan(acc).any(), name
    # any other epilogue with a mask is refused; without one it runs
    mask = _masks(M, dev)["random"]
    out = torch.empty(M, N, device=dev)
    assert _call_masked(a, frags, N, K, g3.EPI_BIAS_RELU, bias, None, mask, out) == -1
    assert _call_masked(a, frags, N, K, g3.EPI_MASK, None, aux, mask, out) == -1
    assert _call_masked(a, frags, N, K, g3.EPI_BIAS_RELU, bias, None, None, out) == 0


def test_masked_panel_with_second_operand_and_python_layer():
    """``gemm_f16x2_panel(..., row_mask=)`` with the query's second operand; the tiled path (``USE_PANEL`` off) gives the same
    values with one ``masked_fill_``."""
    dev = torch.device("cuda")
    torch.manual_seed(5)
    M, N, K = 5000, 256, 256
    w = torch.randn(N, K, device=dev) * 0.05
    a, add = torch.randn(M, K, device=dev), torch.randn(M, K, device=dev)
    bias = torch.randn(N, device=dev)
    mask = _masks(M, dev)["runs"]
    frags = g3.split_frags_f16x2(w, False)
    want = g3.gemm_f16x2_panel(a, frags, N, g3.EPI_BIAS, bias=bias, add=add).masked_fill_(mask[:, None], 0.0)
    got = g3.gemm_f16x2_panel(a, frags, N, g3.EPI_BIAS, bias=bias, add=add, row_mask=mask)
    assert torch.equal(got, want)
    # the cached helpers, panel and tiled
    from ziragroundingdino_amd import transformer
    owner = torch.nn.Linear(K, N).to(dev)
    old = transformer.Switches.gemm_arith
    try:
        transformer.Switches.gemm_arith = "f16x2"
        for panel in (True, False):
            g3.USE_PANEL = panel
            owner.__dict__.pop("_bf16x3_split", None)
            ref = g3.linear(owner, "w", a, w, bias)
            got = g3.linear(owner, "w", a, w, bias, row_mask=mask)
            assert torch.equal(got, ref.masked_fill(mask[:, None], 0.0)), panel
            acc = torch.randn(M, K, device=dev)
            g = torch.randn(M, N, device=dev)
            want = g3.linear_input_grad(owner, "w", g.masked_fill(mask[:, None], 0.0), w, accumulate_into=acc.clone())
            got = g3.linear_input_grad(owner, "w", g, w, accumulate_into=acc.clone(), row_mask=mask)
            assert torch.equal(got, want), panel
            assert torch.equal(got[mask], acc[mask]), panel
    finally:
        g3.USE_PANEL = True
        transformer.Switches.gemm_arith = old


# ---- 2. / 3. the padded encoder node --------------------------------------------------------------------------------------------

SHAPES = [(25, 34), (13, 17), (7, 9), (4, 5)]


def _layer_and_inputs(dev, B=2):
    from ziragroundingdino_amd import transformer
    torch.manual_seed(0)
    layer = transformer.DeformableTransformerEncoderLayer(256, 2048, 0.0, "relu", 4, 8, 4).to(dev).train()
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if "sampling_offsets" in name:
                continue
            p.normal_(0, 0.05) if p.dim() > 1 else p.normal_(0, 0.1)
        layer.norm1.weight.add_(1.0)
        layer.norm2.weight.add_(1.0)
    for p in layer.parameters():
        p.requires_grad_(False)
    S = sum(h * w for h, w in SHAPES)
    g = torch.Generator(device="cpu").manual_seed(1)
    src = torch.randn(B, S, 256, generator=g).to(dev).requires_grad_(True)
    pos = torch.randn(B, S, 256, generator=g).to(dev)
    sh = torch.tensor(SHAPES, device=dev)
    start = torch.cat([sh.new_zeros(1), (sh[:, 0] * sh[:, 1]).cumsum(0)[:-1]])
    # image 1 padded on every level: its bottom rows and right columns
    masks = []
    for h, w in SHAPES:
        m = torch.zeros(B, h, w, dtype=torch.bool)
        m[1, (4 * h + 4) // 5:, :] = True
        m[1, :, (4 * w + 4) // 5:] = True
        masks.append(m.flatten(1))
    mask = torch.cat(masks, 1).to(dev)
    valid = [(~m.view(B, h, w)) for m, (h, w) in zip(masks, SHAPES)]
    ratios = torch.stack([torch.stack([v[:, 0, :].sum(1).float() / w, v[:, :, 0].sum(1).float() / h], -1)
                          for v, (h, w) in zip(valid, SHAPES)], 1).to(dev)
    ref = transformer.TransformerEncoder.get_reference_points(SHAPES, ratios, device=dev)
    gout = torch.randn(B, S, 256, generator=g).to(dev)
    return layer, src, pos, ref, sh, start, mask, gout


def test_padded_applies(monkeypatch):
    from ziragroundingdino_amd import dense
    from ziragroundingdino_amd import encoder_layer as native
    monkeypatch.setattr(dense, "LN_MIN_ROWS", 1)    # (the node takes the row LayerNorm kernel only where the modules do)
    dev = torch.device("cuda")
    layer, src, pos, ref, sh, start, mask, _ = _layer_and_inputs(dev)
    assert native.padded_applies(layer, src, pos, ref, sh, mask)
    assert not native.applies(layer, src, pos, ref, sh, mask)
    assert not native.padded_applies(layer, src, pos, ref, sh, None)
    assert not native.padded_applies(layer, src, pos, ref, sh, mask[:, :-1])           # wrong shape
    assert not native.padded_applies(layer, src, pos, ref, sh, mask[:1])
    assert not native.padded_applies(layer, src, pos, ref, sh, mask.to(torch.uint8))   # not a bool mask
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not native.padded_applies(layer, src, pos, ref, sh, mask)
    cpu = lambda t: t.detach().cpu()
    layer_cpu = _layer_and_inputs(torch.device("cuda"))[0].cpu()
    assert not native.padded_applies(layer_cpu, cpu(src), cpu(pos), cpu(ref), cpu(sh), cpu(mask))
    layer.self_attn.value_proj.weight.requires_grad_(True)                               # trainable weight
    assert not native.padded_applies(layer, src, pos, ref, sh, mask)


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2"])
def test_padded_node_matches_modules(arith, monkeypatch):
    from ziragroundingdino_amd import dense, transformer
    from ziragroundingdino_amd import encoder_layer as native
    monkeypatch.setattr(dense, "LN_MIN_ROWS", 1)    # (the node takes the row LayerNorm kernel only where the modules do)
    monkeypatch.setattr(transformer.Switches, "gemm_arith", arith)
    dev = torch.device("cuda")
    layer, src, pos, ref, sh, start, mask, gout = _layer_and_inputs(dev)
    calls = []
    orig = native.attention_sublayer
    monkeypatch.setattr(native, "attention_sublayer", lambda *a, **k: (calls.append(k.get("key_padding_mask")), orig(*a, **k))[1])

    def run(padded_node, m):
        monkeypatch.setattr(transformer.DeformableTransformerEncoderLayer, "native_padded", padded_node)
        out = layer(src, pos, ref, sh, start, m)[0]
        (gs,) = torch.autograd.grad(out, [src], gout)
        return out, gs

    got = run(True, mask)
    assert len(calls) == 1 and calls[0] is mask
    want = run(False, mask)
    assert len(calls) == 1                          # (the module path)
    assert _rel(got[0], want[0]) < 2e-5, _rel(got[0], want[0])
    assert _rel(got[1], want[1]) < 2e-4, _rel(got[1], want[1])
    # an all-False mask: bit for bit the unpadded node
    none = torch.zeros_like(mask)
    a = run(True, none)
    b = run(True, None)
    assert len(calls) == 3 and calls[1] is none and calls[2] is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. the decoder's value projections ----------------------------------------------------------------------------------------

def test_multi_value_projections_mask_in_the_gemm(monkeypatch):
    from ziragroundingdino_amd import transformer
    from ziragroundingdino_amd.ms_deform_attn import MultiScaleDeformableAttention, multi_value_projections
    monkeypatch.setattr(transformer.Switches, "gemm_arith", "f16x2")
    dev = torch.device("cuda")
    torch.manual_seed(3)
    mods = [MultiScaleDeformableAttention(256, 8, 4, 4, batch_first=True).to(dev) for _ in range(3)]
    for m in mods:
        with torch.no_grad():
            m.value_proj.weight.normal_(0, 0.05)
            m.value_proj.bias.normal_(0, 0.1)
        for p in m.parameters():
            p.requires_grad_(False)
    B, S = 2, 3000
    x = torch.randn(B, S, 256, device=dev)
    mask = torch.zeros(B, S, dtype=torch.bool, device=dev)
    mask[1, 2100:] = True
    mask[1, 700:760] = True
    gos = [torch.randn(B, S, 256, device=dev) for _ in mods]
    launches = []
    real = g3.gemm_f16x2_panel
    monkeypatch.setattr(g3, "gemm_f16x2_panel", lambda *a, **k: (launches.append(k.get("row_mask") is not None), real(*a, **k))[1])

    def run(in_node):
        src = x.clone().requires_grad_(True)
        if in_node:
            outs = multi_value_projections(mods, src, mask)
        else:
            outs = [o.masked_fill(mask[..., None], 0.0) for o in multi_value_projections(mods, src, None)]
        (gx,) = torch.autograd.grad(outs, [src], gos)
        return outs, gx

    got = run(True)
    assert launches == [True] * 6
    want = run(False)
    for o, w in zip(got[0], want[0]):
        assert torch.equal(o, w)
    assert torch.equal(got[1], want[1])
    assert float(got[1][mask].abs().max()) == 0.0


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------

def _ragged_batch():
    from ziragroundingdino_amd.train import synthetic_batch
    a = synthetic_batch(1, 224, 320, n_categories=4, boxes_per_image=3, seed=1, device="cuda")[0]
    b = synthetic_batch(1, 192, 256, n_categories=2, boxes_per_image=2, seed=2, device="cuda")[0]
    return [a, b]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphs"])
def test_ragged_batch_takes_the_padded_node(use_graph, monkeypatch):
    from test_model_gpu import small_model

    from ziragroundingdino_amd import dense
    from ziragroundingdino_amd import encoder_layer as native
    from ziragroundingdino_amd import graphs as zg
    from ziragroundingdino_amd.train import ZiraTrainer
    monkeypatch.setattr(dense, "LN_MIN_ROWS", 1)    # (at this size the node's LayerNorm condition declines otherwise)
    monkeypatch.setattr(zg.GraphedTransformer, "graph_encoder", True)
    model = small_model().train()
    model.use_transformer_graph = use_graph
    trainer = ZiraTrainer(model)
    calls = []
    orig = native.attention_sublayer
    monkeypatch.setattr(native, "attention_sublayer",
                        lambda layer, *a, **k: (calls.append((id(layer), k.get("key_padding_mask") is not None)),
                                                orig(layer, *a, **k))[1])
    data = _ragged_batch()
    enc_layers = [id(layer) for layer in model.transformer.encoder.layers]
    losses = []
    for step in range(3):
        out = trainer.run_step(data)
        assert all(torch.isfinite(v) for v in out.values()), out
        losses.append(float(sum(out.values())))
        if step == 0:
            # every encoder layer ran the padded node (under graphs: while the pieces were captured)
            assert calls and all(padded for _, padded in calls), calls
            if use_graph:
                assert sorted(set(c[0] for c in calls)) == sorted(enc_layers), calls
            else:
                assert sorted(c[0] for c in calls) == sorted(enc_layers), calls
    if not use_graph:
        assert len(calls) == 3 * len(enc_layers)
    torch.cuda.synchronize()
