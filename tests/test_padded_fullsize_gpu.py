"""Full-size pin of a PADDED minibatch: this package's Transformer + heads at BASELINE configs[1] size, frozen, on the GPU,
against the REFERENCE run on the CPU (tests/golden/gen_fullsize_padded_golden.py): image 1 is 640 x 1066 in the 800 x 1333
canvas (padding masks on every level) and its caption has 20 valid tokens of 32.  The padded encoder layers run as the fused
attention node (encoder_layer.padded_applies), the decoder's value projections with the row mask in their GEMMs.

Image 1's top 900 proposals end in a tie: fewer than 900 of its valid proposals score above 0, and every invalid one
(padding, or outside (0.01, 0.99)) scores exactly 0 -- zero memory row, +inf proposal, so all of them carry the same
content and WHICH of them fill the top 900 changes nothing downstream.  The selection is compared on the proposals that
score above the tie; the tied ones only have to be invalid ones.  The helpers are those of test_fullsize_gpu.py."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from gen_fullsize_golden import attach_heads, objective  # noqa: E402
from gen_fullsize_padded_golden import make_padded_inputs  # noqa: E402
from seeded import fill_by_name_, layernorm_weights_plus_one_  # noqa: E402

from ziragroundingdino_amd import transformer, utils  # noqa: E402

TOL = 1e-3


def close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    assert err <= tol, "%s: max err %.3e (scaled by %.3g) > %.1e" % (what, err, scale, tol)


def close_most(a, b, tol, what, frac=0.999, hard=10.0):
    """Elementwise gradients of the full-size model: a sampling location within an ulp of a pixel border falls on
    different sides of `floor` on the two machines, and the piecewise-constant grad_sampling_loc of that ONE sample
    then moves a few elements of a coarse-level gradient by much more than rounding does (measured at B = 2: one
    element of grad srcs[3] at 1.9e-2 of the scale, everything else below 5e-3; the same with round 2's kernels).
    So: `frac` of the elements within `tol`, every element within `hard` x `tol`."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = (a - b).abs() / scale
    ok = float((err <= tol).float().mean())
    assert ok >= frac, "%s: only %.5f of the elements within %.1e" % (what, ok, tol)
    assert float(err.max()) <= hard * tol, "%s: max err %.3e (scaled by %.3g) > %.1e" % (what, float(err.max()), scale, hard * tol)


def count_forward_calls(monkeypatch, fn_class, counts, key):
    """Count the executions of an autograd Function (its ``forward`` static method is looked up on the class at every
    ``apply``)."""
    real = fn_class.forward

    def counted(*a, **k):
        counts[key] = counts.get(key, 0) + 1
        return real(*a, **k)

    monkeypatch.setattr(fn_class, "forward", staticmethod(counted))


def _invalid_proposals(masks, shapes):
    """[B, S] True where the two-stage proposal is invalid (padding, or its box outside (0.01, 0.99))."""
    mask_flat = torch.cat([m.flatten(1) for m in masks], 1)
    _, prop = utils.gen_encoder_output_proposals(torch.zeros(*mask_flat.shape, 1, device=mask_flat.device), mask_flat,
                                                 [tuple(s) for s in shapes])
    return prop.isinf().any(-1).cpu()


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2"])
def test_full_size_padded_transformer_matches_reference(monkeypatch, arith):
    from ziragroundingdino_amd import decoder_layer, encoder_layer

    monkeypatch.setattr(transformer.Switches, "gemm_arith", arith)
    g = torch.load(os.path.join(HERE, "golden", "full_transformer_padded.pt"), weights_only=False)
    st = g["strides"]
    tr = attach_heads(transformer.Transformer(**g["kwargs"]), utils.MLP, utils.ContrastiveEmbed)
    assert [n for n, _ in tr.named_parameters()] == g["param_names"]
    fill_by_name_(tr, g["salt"], g["scale"], g["scales"])
    layernorm_weights_plus_one_(tr)
    tr.to("cuda").eval()
    counts = {}
    for key, cls in (("decoder_layer", decoder_layer._FrozenDecoderLayer), ("decoder_glue", decoder_layer._RefineAndNorm),
                     ("encoder_attention", encoder_layer._FrozenEncoderAttention), ("encoder_ffn", transformer._FrozenFFNNorm)):
        count_forward_calls(monkeypatch, cls, counts, key)
    for p in tr.parameters():
        p.requires_grad_(False)
    srcs, poss, masks, text, tmask, pid, may, gos = make_padded_inputs()
    dev = lambda x: [t.cuda() for t in x] if isinstance(x, list) else x.cuda()
    srcs = [s.requires_grad_(True) for s in dev(srcs)]
    text = dev(text).requires_grad_(True)
    masks, poss, gos = dev(masks), dev(poss), dev(gos)
    invalid = _invalid_proposals(masks, g["shapes"])

    def run():
        text_dict = {"encoded_text": text, "text_token_mask": dev(tmask), "position_ids": dev(pid),
                     "text_self_attention_masks": dev(may)}
        return tr(srcs, masks, None, poss, None, None, text_dict), text_dict

    # 1. two-stage selection: above the tie at 0 the same proposals as a set, near-ties may swap; the tied rest invalid ones
    with torch.no_grad():
        run()
    want_all = g["topk_proposals"]
    assert want_all.shape[0] == 2
    for b in range(2):
        mine, want = tr.last_topk_proposals[b].cpu(), want_all[b]
        srt = g["score_sorted_top1200"][b]
        n = int((srt[:900] > 0).sum())           # (the reference's scores; 900 for image 0, fewer for image 1)
        assert n >= 400, n
        assert torch.equal(mine[:n].sort()[0], want[:n].sort()[0]), b
        assert bool(invalid[b][mine[n:]].all()) and bool(invalid[b][want[n:]].all()), b
        moved = (mine[:n] != want[:n]).nonzero().flatten()
        assert len(moved) <= 40
        for i in moved.tolist():
            gap = min(float(srt[i - 1] - srt[i]) if i else 1.0, float(srt[i] - srt[i + 1]))
            assert gap < 1e-4, (b, i, srt[max(i - 2, 0):i + 3])

    # 1b. the package's own top-k order: rows whose proposal matches the reference's (or both are invalid ones) match its rows
    with torch.no_grad():
        (hs_n, refs_n, hs_enc_n, _, _, _), _ = run()
    mine = tr.last_topk_proposals.cpu()
    same = (mine == want_all) | (torch.gather(invalid, 1, mine) & torch.gather(invalid, 1, want_all))
    scale_h = max(1.0, float(g["hs_last"].abs().max()))
    row_err = ((hs_n[-1][..., ::st["hs_last_channels"]].float().cpu() - g["hs_last"]).abs().amax(-1) / scale_h)
    assert float(same.float().mean()) >= 1 - 40 / 900
    assert float(row_err[same].median()) <= 1e-3 and float(row_err[same].max()) <= 2e-2, (float(row_err[same].median()), float(row_err[same].max()))
    close(objective(hs_n, refs_n, hs_enc_n, gos), g["total"], 2 * TOL, "objective with the package's own top-k order")

    # 2. everything downstream with the reference's order
    real_topk = torch.topk

    def topk_like_reference(x, k, *a, **kw):
        if k == 900 and x.shape[-1] == sum(h * w for h, w in g["shapes"]):
            idx = want_all.to(x.device)
            return torch.gather(x, 1, idx), idx
        return real_topk(x, k, *a, **kw)

    monkeypatch.setattr(torch, "topk", topk_like_reference)
    counts.clear()
    (hs, refs, hs_enc, ref_enc, init_box, _), text_dict = run()
    assert torch.equal(tr.last_topk_proposals.cpu(), want_all)
    close(text_dict["encoded_text"], g["memory_text"], TOL, "memory_text")
    close(hs[-1][..., ::st["hs_last_channels"]], g["hs_last"], TOL, "hs[-1]")
    close(hs[0][:, ::st["hs_queries"]], g["hs_first_sample"], TOL, "hs[0] sample")
    close(refs[-1], g["reference_last"], TOL, "references[-1]")
    close(hs_enc[:, :, ::st["hs_queries"]], g["hs_enc_sample"], TOL, "hs_enc sample")
    close(ref_enc, g["ref_enc"], TOL, "ref_enc")
    total = objective(hs, refs, hs_enc, gos)
    close(total, g["total"], TOL, "objective")
    grads = torch.autograd.grad(total, srcs + [text])
    GTOL = 5e-3
    close(torch.stack([x.norm() for x in grads[:4]]), g["grad_src_norms"], TOL, "grad src norms")
    close(grads[4].norm(), g["grad_text"].norm(), TOL, "grad text norm")
    close_most(grads[4], g["grad_text"], GTOL, "grad text")
    close_most(grads[3][:, ::st["grad_src3_channels"]], g["grad_src3"], GTOL, "grad srcs[3]", frac=0.995)
    close_most(grads[0][:, ::8, ::10, ::10], g["grad_src0_sample"], GTOL, "grad srcs[0] sample")
    # the padded batch ran through the one-node forms, six layers each
    assert counts == {"decoder_layer": 6, "decoder_glue": 6, "encoder_attention": 6, "encoder_ffn": 6}, counts
