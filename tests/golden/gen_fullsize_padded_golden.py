"""Full-size pin of the transformer on a PADDED minibatch against the REFERENCE (companion of gen_fullsize_golden.py).

Same model, weights (``SALT``), inputs and stored keys as ``full_transformer.pt``, but the batch is what an ODinW task
minibatch looks like: image 0 fills the 800 x 1333 canvas, image 1 is 640 x 1066 inside it, and its four level masks are the
nearest-neighbour ``F.interpolate`` of the pixel mask, as the reference's backbone makes them
(backbone/swin_transformer.py:751).  Image 1's caption has 20 valid tokens of 32: the padded ones are masked in
``text_token_mask``, attend only to themselves in ``text_self_attention_masks`` and have position id 0.
The larger outputs are stored at a coarser stride than in ``full_transformer.pt`` (``SAMPLE``, kept in the fixture under
``strides``) so that the file stays under 1 MiB.  ~2 min of CPU time, ~20 GB of memory.

    python tests/golden/gen_fullsize_padded_golden.py      (needs the reference checkout; never runs on the GPU box)
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_fullsize_golden import SALT, SCALES, SHAPES, attach_heads, full_args, make_inputs, objective  # noqa: E402

CANVAS = (800, 1333)
IMAGE1 = (640, 1066)      # (height, width) of image 1's valid pixels, top-left in the canvas
NTOK_VALID1 = 20          # valid caption tokens of image 1
# strides of the stored samples: channels of hs[-1], queries of hs[0] and hs_enc, tokens of the memory, channels of grad srcs[3]
SAMPLE = dict(hs_last_channels=8, hs_queries=18, memory_tokens=388, grad_src3_channels=4)


def make_padded_inputs(d=256):
    """``make_inputs()`` with image 1 and its caption padded (the test calls this too: nothing of it is stored)."""
    srcs, poss, masks, text, tmask, pid, may, gos = make_inputs(d)
    pixel = torch.zeros(1, *CANVAS, dtype=torch.bool)
    pixel[:, IMAGE1[0]:, :] = True
    pixel[:, :, IMAGE1[1]:] = True
    masks = [m.clone() for m in masks]
    for m, (h, w) in zip(masks, SHAPES):
        m[1] = F.interpolate(pixel[None].float(), size=(h, w)).to(torch.bool)[0, 0]
    n = NTOK_VALID1
    tmask, pid, may = tmask.clone(), pid.clone(), may.clone()
    tmask[1, n:] = False
    pid[1, n:] = 0
    may[1, n:, :] = False
    may[1, :, n:] = False
    idx = torch.arange(n, tmask.shape[1])
    may[1, idx, idx] = True
    return srcs, poss, masks, text, tmask, pid, may, gos


def main():
    import ref_import
    from seeded import fill_by_name_, layernorm_weights_plus_one_

    torch.set_num_threads(os.cpu_count() or 1)
    ref = ref_import.load()
    T_, U = ref["transformer_for_adapter"], ref["utils"]
    tr = attach_heads(T_.Transformer(**full_args()), U.MLP, U.ContrastiveEmbed)
    fill_by_name_(tr, SALT, 0.05, SCALES)
    layernorm_weights_plus_one_(tr)
    tr.eval()
    srcs, poss, masks, text, tmask, pid, may, gos = make_padded_inputs()
    srcs = [s.requires_grad_(True) for s in srcs]
    text = text.requires_grad_(True)
    text_dict = {"encoded_text": text, "text_token_mask": tmask, "position_ids": pid,
                 "text_self_attention_masks": may}
    hs, refs, hs_enc, ref_enc, init_box, _ = tr(srcs, masks, None, poss, None, None, dict(text_dict))
    total = objective(hs, refs, hs_enc, gos)
    grads = torch.autograd.grad(total, srcs + [text])
    with torch.no_grad():  # the two-stage selection, recomputed as transformer_for_adapter.py:301-318 does
        src_flat = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
        mask_flat = torch.cat([m.flatten(1) for m in masks], 1)
        pos_flat = torch.cat([p.flatten(2).transpose(1, 2) + tr.level_embed[i].view(1, 1, -1)
                              for i, p in enumerate(poss)], 1)
        sh = torch.tensor(SHAPES)
        lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
        vr = torch.stack([tr.get_valid_ratio(m) for m in masks], 1)
        memory, memory_text, _ = tr.encoder(src_flat, pos=pos_flat, level_start_index=lsi, spatial_shapes=sh,
                                            valid_ratios=vr, key_padding_mask=mask_flat, memory_text=text,
                                            text_attention_mask=~tmask, position_ids=pid,
                                            text_self_attention_masks=may)
        om, _ = U.gen_encoder_output_proposals(memory, mask_flat, sh)
        om_raw = om
        om = tr.enc_output_norm(tr.enc_output(om))
        logits = tr.enc_out_class_embed(om, {"encoded_text": memory_text, "text_token_mask": tmask})
        score = logits.max(-1)[0]
        topk = torch.topk(score, 900, dim=1)[1]
        srt = torch.sort(score, dim=1, descending=True)[0]
    out = dict(
        kwargs=full_args(), salt=SALT, scale=0.05, scales=SCALES, shapes=SHAPES, strides=dict(SAMPLE),
        param_names=[n for n, _ in tr.named_parameters()],
        topk_proposals=topk, score_900th_gap=(srt[:, 899] - srt[:, 900]), score_scale=srt[:, 0] - srt[:, -1],
        score_min_gap_top900=(srt[:, :900] - srt[:, 1:901]).min(), score_sorted_top1200=srt[:, :1200].clone(),
        score_of_invalid=score[0][(om_raw.abs().sum(-1) == 0)[0]][:4].clone(), n_invalid=int((om_raw.abs().sum(-1) == 0).sum()),
        memory_sample=memory[:, ::SAMPLE["memory_tokens"]].clone(), memory_text=memory_text.clone(),
        hs_last=hs[-1][..., ::SAMPLE["hs_last_channels"]].detach().clone(),
        hs_first_sample=hs[0][:, ::SAMPLE["hs_queries"]].detach().clone(),
        reference_last=refs[-1].detach().clone(), hs_enc_sample=hs_enc[:, :, ::SAMPLE["hs_queries"]].detach().clone(),
        ref_enc=ref_enc.detach().clone(), total=total.detach(),
        grad_text=grads[4].clone(), grad_src_norms=torch.stack([g.norm() for g in grads[:4]]),
        grad_src3=grads[3][:, ::SAMPLE["grad_src3_channels"]].clone(), grad_src0_sample=grads[0][:, ::8, ::10, ::10].clone())
    path = os.path.join(HERE, "full_transformer_padded.pt")
    torch.save(out, path)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3), "| total %.6f" % float(total.detach()),
          "| 900th-901st score gap %s, smallest gap inside the top 900 %.3e (scale %s)"
          % (out["score_900th_gap"].tolist(), float(out["score_min_gap_top900"]), out["score_scale"].tolist()))


if __name__ == "__main__":
    main()
