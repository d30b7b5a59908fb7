"""Loss functions on the metric path: compute_mlm / compute_itm / compute_itm_hardneg / compute_itc / compute_vqa /
compute_caption_mle / compute_caption_cider + caption_test_step / caption_test_wrapup / init_weights (reference
coarse_grained/fiber/modules/objectives.py:17-213, 502-510, 560-896).  Same call signatures and return keys."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def _mlm_ce(logits, labels, head=None, owner=None):
    """F.cross_entropy(logits, labels, ignore_index=-100) (objectives.py:24-28) on the HIP kernel for bf16 device logits.

    The 50265-way logits are bf16 (2 B instead of 8 MB per sample of HBM traffic); log-sum-exp averages their rounding away,
    but the LABEL logit enters the loss directly, and 2^-9 relative rounding of a logit of magnitude 5-10 is 1e-2..2e-2 per
    token -- the dominant term of the loss-curve gap to the fp32 reference (tests/test_hip_modules.py, 50-step curve).  With
    `head` (the MLMHead, after its forward) the label logit is recomputed in fp32 from the head's hidden state -- a gathered
    dot product per token -- and substituted into the loss VALUE; gradients are unchanged (they are the same function)."""
    x16 = logits.to(torch.bfloat16)
    loss = ops.cross_entropy(x16, labels, -100)
    if owner is not None and getattr(x16, "_fiber_argmax", None) is not None:
        owner._fiber_argmax = x16._fiber_argmax              # the arg max of the labelled rows rides on the logits the metric will be given
    if head is not None and head.last_hidden is not None:
        with torch.no_grad():
            h = head.last_hidden.reshape(-1, head.last_hidden.shape[-1])
            valid = labels != -100
            lab = labels.clamp(min=0)
            z16 = logits.gather(1, lab[:, None]).squeeze(1).float()
            z32 = (h.float() * head.decoder.weight[lab]).sum(-1) + head.bias[lab]
            corr = ((z16 - z32) * valid).sum() / valid.sum().clamp(min=1)
        loss = loss + corr                                  # a constant w.r.t. autograd: value correction only
    return loss


def _mlm_head(pl_module, text_feats, labels):
    """MLM head + loss (objectives.py:17-33: `mlm_score(text_feats)`, cross entropy with ignore_index -100).

    85 % of the rows carry the ignore label: the reference still pushes them through the 50265-way decoder (forward, dX, dW) and
    writes a zero gradient row for each.  With `mlm_compact_rows` (default OFF: the reference's output shapes) only the rows that carry a label go through the head:
    same loss (the mean runs over labelled rows either way), same gradients (an ignored row's logit gradient is exactly zero), same
    accuracy (the metric drops ignored rows).  The row count is data dependent, so the selection costs ONE host sync per step; it is
    skipped while a hipGraph is being captured (static shapes) and when no row is labelled.  Returns (loss, logits, labels) --
    the logits / labels of the labelled rows only ([n, V] / [n]) on the compact path, the full tensors otherwise."""
    cfg = pl_module.hparams.config
    V = cfg["vocab_size"]
    flat = labels.reshape(-1)
    if cfg.get("mlm_compact_rows", False) and text_feats.is_cuda and not torch.cuda.is_current_stream_capturing():
        keep = (flat != -100).nonzero(as_tuple=True)[0]
        if keep.numel() > 0:
            feats = text_feats.reshape(-1, text_feats.shape[-1]).index_select(0, keep)
            lab = flat.index_select(0, keep)
            logits = pl_module.mlm_score(feats)
            return _mlm_ce(logits, lab, pl_module.mlm_score, owner=logits), logits, lab
    logits = pl_module.mlm_score(text_feats)
    return _mlm_ce(logits.view(-1, V), flat, pl_module.mlm_score, owner=logits), logits, labels


def compute_mlm(pl_module, batch):
    infer = pl_module.infer(batch, mask_text=True, mask_image=False)
    mlm_loss, mlm_logits, mlm_labels = _mlm_head(pl_module, infer["text_feats"], infer["text_labels"])
    ret = {"mlm_loss": mlm_loss, "mlm_logits": mlm_logits, "mlm_labels": mlm_labels, "mlm_ids": infer["text_ids"]}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_mlm_loss")(ret["mlm_loss"])
    acc = getattr(pl_module, f"{phase}_mlm_accuracy")(ret["mlm_logits"], ret["mlm_labels"])
    pl_module.log(f"mlm/{phase}/loss", loss)
    pl_module.log(f"mlm/{phase}/accuracy", acc)
    return ret


def compute_itm(pl_module, batch, itm_labels=None):
    """`itm_labels` (optional) pins the true/false permutation for parity tests; by default it is drawn with
    torch.randperm exactly as the reference does (objectives.py:47-48)."""
    pos_len = len(batch["text"]) // 2
    neg_len = len(batch["text"]) - pos_len
    if itm_labels is None:
        itm_labels = torch.cat([torch.ones(pos_len), torch.zeros(neg_len)]).to(pl_module.device)
        itm_labels = itm_labels[torch.randperm(itm_labels.size(0))]
    else:
        itm_labels = itm_labels.to(pl_module.device).float()
    sel = itm_labels.view(-1, 1, 1, 1) == 1
    itm_images = [torch.where(sel, bti, bfi) for bti, bfi in zip(batch["image"], batch["false_image_0"])]
    batch = {k: v for k, v in batch.items()}
    batch["image"] = itm_images
    infer = pl_module.infer(batch, mask_text=False, mask_image=False)
    itm_logits = pl_module.itm_score(infer["cls_feats"])
    itm_loss = F.cross_entropy(itm_logits, itm_labels.long())
    ret = {"itm_loss": itm_loss, "itm_logits": itm_logits, "itm_labels": itm_labels}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_itm_loss")(ret["itm_loss"])
    acc = getattr(pl_module, f"{phase}_itm_accuracy")(ret["itm_logits"], ret["itm_labels"])
    pl_module.log(f"itm/{phase}/loss", loss)
    pl_module.log(f"itm/{phase}/accuracy", acc)
    return ret


def compute_mlm_itm_fused(pl_module, batch, itm_labels=None):
    """compute_mlm + compute_itm (objectives.py:17-75) evaluated in ONE fused-backbone pass over the 2B concatenated
    samples [masked-text pairs ; true/false-image pairs].  Every op on the path is per-sample (LayerNorm, window /
    cross attention, per-sample DropPath), so the two halves are exactly the two separate infer() calls of the
    reference; one pass halves the kernel-launch count and doubles the GEMM M dimension.  Same return keys."""
    B = len(batch["text"])
    pos_len = B // 2
    if itm_labels is None:
        itm_labels = torch.cat([torch.ones(pos_len), torch.zeros(B - pos_len)]).to(pl_module.device)
        itm_labels = itm_labels[torch.randperm(itm_labels.size(0))]
    else:
        itm_labels = itm_labels.to(pl_module.device).float()
    true_img, false_img = batch["image"][0], batch["false_image_0"][0]
    fused = {
        # [true ; where(label == 1, true, false)] as its two sources: the patch embedding gathers from them (ops.ImagePair)
        "image": [ops.ImagePair(true_img, false_img, itm_labels == 1)],
        "text_ids": torch.cat([batch["text_ids_mlm"], batch["text_ids"]], 0),
        "text_labels": torch.cat([batch["text_labels_mlm"], batch["text_labels"]], 0),
        "text_masks": torch.cat([batch["text_masks"], batch["text_masks"]], 0),
    }
    infer = pl_module.infer(fused, mask_text=False, mask_image=False)
    mlm_loss, mlm_logits, mlm_labels = _mlm_head(pl_module, infer["text_feats"][:B], batch["text_labels_mlm"])
    itm_logits = pl_module.itm_score(infer["cls_feats"][B:])
    itm_loss = F.cross_entropy(itm_logits, itm_labels.long())
    ret = {"mlm_loss": mlm_loss, "mlm_logits": mlm_logits, "mlm_labels": mlm_labels, "mlm_ids": batch["text_ids_mlm"],
           "itm_loss": itm_loss, "itm_logits": itm_logits, "itm_labels": itm_labels}
    phase = "train" if pl_module.training else "val"
    for task in ("mlm", "itm"):
        loss = getattr(pl_module, f"{phase}_{task}_loss")(ret[f"{task}_loss"])
        acc = getattr(pl_module, f"{phase}_{task}_accuracy")(ret[f"{task}_logits"], ret[f"{task}_labels"])
        pl_module.log(f"{task}/{phase}/loss", loss)
        pl_module.log(f"{task}/{phase}/accuracy", acc)
    return ret


def compute_itc(pl_module, batch, neg_override=None):
    """Image-text contrastive loss against the local batch + the feature queues, and the hard-negative draw that feeds
    compute_itm_hardneg (objectives.py:119-180, after ALBEF).  The reference draws one negative per row with a Python loop
    of `torch.multinomial(...).item()` (2B host syncs); here both draws are one batched multinomial each and the gathers stay
    on the device -- the same distribution, a different consumption of the RNG stream.  `neg_override = (image_idx, text_idx)`
    pins the draw for parity tests."""
    with torch.no_grad():
        pl_module.temp.clamp_(0.001, 1.0)
    infer_image = pl_module.infer(batch, mask_image=False, mask_text=False, image_only=True)
    infer_text = pl_module.infer(batch, mask_image=False, mask_text=False, text_only=True)
    image_feat, text_feat = infer_image["cls_feats"].float(), infer_text["cls_feats"].float()
    image_feat_all = torch.cat([image_feat.t().detach(), pl_module.image_queue.detach().float()], dim=1)
    text_feat_all = torch.cat([text_feat.t().detach(), pl_module.text_queue.detach().float()], dim=1)
    sim_i2t = ops.lib_linear(image_feat, text_feat_all.t().contiguous()) / pl_module.temp
    sim_t2i = ops.lib_linear(text_feat, image_feat_all.t().contiguous()) / pl_module.temp
    bs = image_feat.size(0)
    diag = torch.arange(bs, device=sim_i2t.device)
    loss_i2t = -F.log_softmax(sim_i2t, dim=1)[diag, diag].mean()         # sim_targets = identity on the first bs columns
    loss_t2i = -F.log_softmax(sim_t2i, dim=1)[diag, diag].mean()
    loss_itc = (loss_i2t + loss_t2i) / 2.0

    total = int(pl_module.queue_total)      # NB as in the reference this may exceed queue_size once the queue has wrapped
    pool = min(bs + total, sim_i2t.shape[1])
    tot_image = torch.cat([batch["image"][0], pl_module.image_input_queue[:total].to(batch["image"][0].dtype)], dim=0)
    tot_text = torch.cat([batch["text_ids"], pl_module.text_input_queue[:total]], dim=0)
    tot_text_mask = torch.cat([batch["text_masks"], pl_module.text_input_mask_queue[:total]], dim=0)
    if neg_override is not None:
        img_idx, txt_idx = (torch.as_tensor(v, device=sim_i2t.device) for v in neg_override)
    else:
        with torch.no_grad():
            w_i2t = F.softmax(sim_i2t[:, :pool], dim=1)
            w_t2i = F.softmax(sim_t2i[:, :pool], dim=1)
            w_i2t[diag, diag] = 0
            w_t2i[diag, diag] = 0
            img_idx = torch.multinomial(w_t2i + 1e-9, 1).squeeze(1)
            txt_idx = torch.multinomial(w_i2t + 1e-9, 1).squeeze(1)
    image_neg, text_neg, text_mask_neg = tot_image[img_idx], tot_text[txt_idx], tot_text_mask[txt_idx]

    if pl_module.training:
        pl_module._dequeue_and_enqueue(infer_image["cls_feats"].detach().clone(), infer_text["cls_feats"].detach().clone(),
                                       batch["image"][0].clone(), batch["text_ids"].clone(), batch["text_masks"].clone())
    ret = {"itc_loss": loss_itc}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_itc_loss")(ret["itc_loss"])
    pl_module.log(f"itc/{phase}/loss", loss)
    return ret, image_neg, text_neg, text_mask_neg


def compute_itm_hardneg(pl_module, batch, image_neg, text_neg, text_mask_neg):
    """ITM over 3B pairs: the B true pairs, (image, hard-negative text) and (hard-negative image, text)
    (objectives.py:78-116).  The reference overwrites batch["image"/"text_ids"/"text_masks"] in place; a shallow copy is
    used here so later objectives still see the loader's batch."""
    pos_len = len(batch["text"])
    itm_labels = torch.cat([torch.ones(pos_len), torch.zeros(2 * pos_len)]).to(pl_module.device)
    img = batch["image"][0]
    b3 = {k: v for k, v in batch.items()}
    b3["image"] = [torch.cat([img, img, image_neg.to(img.dtype)], dim=0)]
    b3["text_ids"] = torch.cat([batch["text_ids"], text_neg, batch["text_ids"]], dim=0)
    b3["text_masks"] = torch.cat([batch["text_masks"], text_mask_neg, batch["text_masks"]], dim=0)
    b3["text_labels"] = torch.cat([batch["text_labels"]] * 3, dim=0)
    infer = pl_module.infer(b3, mask_text=False, mask_image=False)
    itm_logits = pl_module.itm_score(infer["cls_feats"])
    itm_loss = F.cross_entropy(itm_logits, itm_labels.long())
    ret = {"itm_loss": itm_loss, "itm_logits": itm_logits, "itm_labels": itm_labels}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_itm_loss")(ret["itm_loss"])
    acc = getattr(pl_module, f"{phase}_itm_accuracy")(ret["itm_logits"], ret["itm_labels"])
    pl_module.log(f"itm/{phase}/loss", loss)
    pl_module.log(f"itm/{phase}/accuracy", acc)
    return ret


def compute_mlm_itm_hardneg_fused(pl_module, batch, image_neg, text_neg, text_mask_neg):
    """compute_mlm + compute_itm_hardneg (objectives.py:17-33, 78-116) in ONE fused-backbone pass over 4B samples
    [B masked-text pairs ; B true pairs ; B (image, hard-negative text) ; B (hard-negative image, text)] -- the same
    per-sample computation as the reference's two infer() calls, with a quarter fewer launches and larger GEMMs."""
    B = len(batch["text"])
    img = batch["image"][0]
    fused = {
        "image": [torch.cat([img, img, img, image_neg.to(img.dtype)], 0)],
        "text_ids": torch.cat([batch["text_ids_mlm"], batch["text_ids"], text_neg, batch["text_ids"]], 0),
        "text_labels": torch.cat([batch["text_labels_mlm"]] + [batch["text_labels"]] * 3, 0),
        "text_masks": torch.cat([batch["text_masks"], batch["text_masks"], text_mask_neg, batch["text_masks"]], 0),
    }
    infer = pl_module.infer(fused, mask_text=False, mask_image=False)
    mlm_loss, mlm_logits, mlm_labels = _mlm_head(pl_module, infer["text_feats"][:B], batch["text_labels_mlm"])
    itm_labels = torch.cat([torch.ones(B), torch.zeros(2 * B)]).to(pl_module.device)
    itm_logits = pl_module.itm_score(infer["cls_feats"][B:])
    itm_loss = F.cross_entropy(itm_logits, itm_labels.long())
    ret = {"mlm_loss": mlm_loss, "mlm_logits": mlm_logits, "mlm_labels": mlm_labels, "mlm_ids": batch["text_ids_mlm"],
           "itm_loss": itm_loss, "itm_logits": itm_logits, "itm_labels": itm_labels}
    phase = "train" if pl_module.training else "val"
    for task in ("mlm", "itm"):
        loss = getattr(pl_module, f"{phase}_{task}_loss")(ret[f"{task}_loss"])
        acc = getattr(pl_module, f"{phase}_{task}_accuracy")(ret[f"{task}_logits"], ret[f"{task}_labels"])
        pl_module.log(f"{task}/{phase}/loss", loss)
        pl_module.log(f"{task}/{phase}/accuracy", acc)
    return ret


def compute_vqa(pl_module, batch):
    """VQAv2 fine-tune head (objectives.py:182-213): soft-target BCE over the answer vocabulary, scaled by its size."""
    infer = pl_module.infer(batch, mask_text=False, mask_image=False)
    vqa_logits = pl_module.vqa_classifier(infer["cls_feats"])
    n_ans = pl_module.hparams.config["vqav2_label_size"]
    vqa_targets = torch.zeros(len(vqa_logits), n_ans, device=vqa_logits.device)
    vqa_labels, vqa_scores = batch["vqa_labels"], batch["vqa_scores"]
    for i, (_label, _score) in enumerate(zip(vqa_labels, vqa_scores)):
        for lab, sc in zip(_label, _score):
            vqa_targets[i, lab] = sc
    vqa_loss = F.binary_cross_entropy_with_logits(vqa_logits.float(), vqa_targets) * vqa_targets.shape[1]
    ret = {"vqa_loss": vqa_loss, "vqa_logits": vqa_logits, "vqa_targets": vqa_targets, "vqa_labels": vqa_labels,
           "vqa_scores": vqa_scores}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_vqa_loss")(ret["vqa_loss"])
    score = getattr(pl_module, f"{phase}_vqa_score")(ret["vqa_logits"], ret["vqa_targets"])
    pl_module.log(f"vqa/{phase}/loss", loss)
    pl_module.log(f"vqa/{phase}/score", score)
    return ret


def vqa_test_step(pl_module, batch, output):
    """objectives.py:513-524: arg-max answer strings for a test batch (answer vocabulary from the datamodule)."""
    dicts = pl_module.trainer.datamodule.dm_dicts
    id2answer = (dicts["vqa_trainval"] if "vqa_trainval" in dicts else dicts["vqa"]).id2answer
    picks = output["vqa_logits"].argmax(dim=-1).tolist()
    return {"qids": batch["qid"], "preds": [id2answer[i] for i in picks]}


def vqa_test_wrapup(outs, model_name, out_dir="result"):
    """objectives.py:531-557: every rank writes its shard, rank 0 merges the shards into result/vqa_submit_<model>.json."""
    import glob
    import json
    import os
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if multi else 0
    records = [{"question_id": q, "answer": a} for out in outs for q, a in zip(out["qids"], out["preds"])]
    shard = f"vqa_submit_{rank}.json"
    with open(shard, "w") as fp:
        json.dump(records, fp, indent=4)
    if multi:
        dist.barrier()
    if rank == 0:
        merged = []
        for path in sorted(glob.glob("vqa_submit_*.json")):
            with open(path) as fp:
                merged += json.load(fp)
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"vqa_submit_{model_name}.json"), "w") as fp:
            json.dump(merged, fp, indent=4)
    if multi:
        dist.barrier()
    os.remove(shard)


def compute_caption_mle(pl_module, batch):
    """objectives.py:682-710: the MLM head over EVERY text position of the causal decoder, labels = the ids shifted left by one and
    padded with pad_token_id, pad -> -100 (ignored); cross entropy through _mlm_head / _mlm_ce like compute_mlm."""
    tok = pl_module.trainer.datamodule.dms[0].tokenizer
    infer = pl_module.infer_caption(batch, mask_text=False, mask_image=False)
    ids = infer["text_ids"]
    labels = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], tok.pad_token_id)], 1)
    labels = labels.masked_fill(labels == tok.pad_token_id, -100)
    loss, logits, labels = _mlm_head(pl_module, infer["text_feats"], labels)
    ret = {"caption_mle_loss": loss, "caption_mle_logits": logits, "caption_mle_labels": labels, "caption_mle_ids": ids}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_caption_mle_loss")(ret["caption_mle_loss"])
    acc = getattr(pl_module, f"{phase}_caption_mle_accuracy")(ret["caption_mle_logits"], ret["caption_mle_labels"])
    pl_module.log(f"caption_mle/{phase}/loss", loss)
    pl_module.log(f"caption_mle/{phase}/accuracy", acc)
    return ret


def _wrap_sentence(s):
    """objectives.py:720-728 (after VinVL): no trailing full stop, and an <eos> word, as the cached CIDEr document frequencies have it."""
    r = s.strip()
    if r.endswith("."):
        r = r[:-1]
    return r + " <eos>"


def _head_logits_2d(pl_module, feats):
    """mlm_score over [N, L, H] features as [N * L, V] rows, bf16 on the device (what the loss.hip kernels read)."""
    logits = pl_module.mlm_score(feats)
    flat = logits.reshape(-1, logits.shape[-1])
    return flat.to(torch.bfloat16) if flat.is_cuda else flat


def _caption_cider_scores(scorer, tok, text_ids, gt_txt, beam_size):
    """objectives.py:830-856: CIDEr-D of every sampled caption (tokenizer.decode without the cls / sep / pad strings, _wrap_sentence) against
    the references of its image (gt_txt[image], the same list for each of its beams): np.ndarray [bs * beam]."""
    strip = (tok.cls_token, tok.sep_token, tok.pad_token)
    res, gts = [], {}
    for i, ids in enumerate(text_ids.tolist()):
        s = tok.decode(ids)
        for t in strip:
            s = s.replace(t, "")
        res.append({"image_id": i, "caption": [_wrap_sentence(s)]})
        gts[i] = [_wrap_sentence(g) for g in gt_txt[i // beam_size]]
    return scorer.compute_score(gts, res)[1]


def _cached_feats(pl_module, image_embeds, beam_size):
    """The per-step features of the two decoding loops from a KV-cached decoder -- anything with .step(tokens [N], parent [N] or None) ->
    [N, H] -- instead of infer_caption on the ids so far: feats_at(i, ids, parent) -> [rows, 1, H] of position i.  Step 0 feeds ids[:, 0]
    ([CLS]) to all bs * beam rows and hands back the first row of each image, as the loops expect bs rows there (beam - 1 redundant
    single-token rows per image, once); later steps feed column i of the already reordered ids, with the reorder as `parent`."""
    decoder = pl_module.caption_decoder(image_embeds, beam_size)

    def feats_at(i, ids, parent):
        if i == 0:
            return decoder.step(ids[:, 0].repeat_interleave(beam_size, 0))[::beam_size, None]
        return decoder.step(ids[:, i], parent)[:, None]
    return feats_at


@torch.no_grad()
def _caption_sample(pl_module, tok, image, image_embeds, beam_size, max_len):
    """objectives.py:730-796: beam_size sampled continuations per image, [bs * beam, max_len] ids laid out image-major.  Step 0 runs on the
    two-token prefix [cls, pad] (with the image tower unless image_embeds is handed in) and draws beam_size tokens per image with replacement;
    every later step re-runs the causal text stack on the ids so far and draws one token per beam, ended beams are padded, and the loop stops
    once all have ended.  The draws are ops.sample_rows (Gumbel-max on the dropout key stream) instead of softmax + torch.multinomial.

    config["caption_decode_cache"]: every step feeds ONE token per beam to pl_module.caption_decoder (an object with .step(tokens, parent),
    modules/caption_decode.py) instead of re-running infer_caption on the ids so far.  The decoder is evaluation arithmetic: in training mode
    the reference samples with dropout on (the module is in train mode), the cached sampler draws from the model WITHOUT dropout -- a stated
    difference, like caption_cider_share_image, and the reason the flag is off by default."""
    bs, dev = image.size(0), image.device
    pad, sep, mask_id = tok.pad_token_id, tok.sep_token_id, tok.mask_token_id
    text_ids = torch.full((bs, max_len), pad, device=dev, dtype=torch.long)
    text_ids[:, 0] = tok.cls_token_id
    if pl_module.hparams.config.get("caption_decode_cache", False):
        feats_at = _cached_feats(pl_module, pl_module.caption_image_embeds(image) if image_embeds is None else image_embeds, beam_size)
    else:
        b = {"image": [image], "text_ids": text_ids[:, :2], "text_labels": None, "text_masks": text_ids[:, :2] != pad}
        first = pl_module.infer_caption(b, mask_text=False, mask_image=False, image_embeds=image_embeds)
        image_embeds = first["image_embeds"].repeat_interleave(beam_size, 0)
        b["text_masks"] = None

        def feats_at(i, ids, parent):
            b["text_ids"] = ids
            infer = first if i == 0 else pl_module.infer_caption(b, mask_text=False, mask_image=False, image_embeds=image_embeds)
            return infer["text_feats"][:, i:i + 1]
    end_seq = None
    for i in range(max_len - 1):
        logits = _head_logits_2d(pl_module, feats_at(i, text_ids, None))
        if i == 0:
            tokens, _, end_seq = ops.sample_rows(logits, beam_size, mask_id, pad_id=pad, sep_id=sep)      # [bs, beam]
            text_ids = text_ids.repeat_interleave(beam_size, 0)
        else:
            tokens, _, end_seq = ops.sample_rows(logits, 1, mask_id, ended=end_seq, pad_id=pad, sep_id=sep)
        text_ids[:, i + 1] = tokens.reshape(-1)
        end_seq = end_seq.reshape(-1)
        if i > 0 and bool(end_seq.all()):
            break
    return text_ids.contiguous()


def compute_caption_cider(pl_module, batch, beam_size=5, alpha=0.3, sampled_ids=None):
    """objectives.py:712-896, self-critical sequence training on CIDEr-D: alpha * caption_loss + (1 - alpha) * rl_loss.  In training, beam_size
    captions per image are sampled without gradient (_caption_sample), scored on the host against batch["gt_txt"] (modules/cider.py), and
    re-scored WITH gradient: rl_loss = sum_seq mean_t log(p(token_t) + 1e-9) * (100 - 100 cider) / bs, the per-token term on ops.seq_logprob
    (csrc/loss.hip) instead of softmax / + 1e-9 / log / gather over [bs * beam * L, V] fp32 tensors; a sequence without any non-pad label adds 0.
    Outside training rl_loss = 0.  caption_loss is compute_caption_mle's term on the batch's own text.  The caller's batch is not modified.

    `sampled_ids` (int64 [bs * beam, max_text_len]) pins the sampled captions for parity tests, like compute_itc's neg_override.
    config["caption_cider_share_image"]: the image tower runs once with gradient (on the batch's images) and its tokens serve the sampling
    (detached), the RL pass (repeated per beam: autograd sums the beams' gradients) and the MLE term, instead of the reference's 1 + beam + 1
    tower samples per image.  Same function of the weights; in training mode each image then gets ONE DropPath draw instead of seven."""
    cfg = pl_module.hparams.config
    tok = pl_module.trainer.datamodule.dms[0].tokenizer
    pad = tok.pad_token_id
    share = bool(cfg.get("caption_cider_share_image", False))
    caption_infer = pl_module.infer_caption(batch, mask_text=False, mask_image=False) if share else None
    rl_loss = 0
    if pl_module.training:
        image = batch["image"][0]
        bs = image.size(0)
        shared = caption_infer["image_embeds"] if share else None
        if sampled_ids is None:
            text_ids = _caption_sample(pl_module, tok, image, shared.detach() if share else None, beam_size, cfg["max_text_len"])
        else:
            text_ids = sampled_ids.to(image.device).contiguous()
        n = text_ids.size(0)
        assert n == bs * beam_size, (n, bs, beam_size)
        batch_rl = {"image": [None if share else image.repeat_interleave(beam_size, 0)], "text_ids": text_ids, "text_labels": None,
                    "text_masks": text_ids != pad}
        infer_rl = pl_module.infer_caption(batch_rl, mask_text=False, mask_image=False,
                                           image_embeds=shared.repeat_interleave(beam_size, 0) if share else None)
        rl_labels = torch.cat([text_ids[:, 1:], torch.full_like(text_ids[:, :1], pad)], 1)
        lp = ops.seq_logprob(_head_logits_2d(pl_module, infer_rl["text_feats"]), rl_labels.reshape(-1), pad).view(n, -1)
        rl_len = (rl_labels != pad).sum(-1).float()
        seq_logp = lp.sum(-1) / (rl_len + 1e-9)                                     # [bs * beam]; 0 for a sequence of pads only

        scores = _caption_cider_scores(pl_module.cider_scorer, tok, text_ids, batch["gt_txt"], beam_size)
        weight = torch.as_tensor(100.0 - 100.0 * scores, dtype=torch.float32).to(seq_logp.device)
        rl_loss = (seq_logp * weight).sum() / bs

    if caption_infer is None:
        caption_infer = pl_module.infer_caption(batch, mask_text=False, mask_image=False)
    ids = caption_infer["text_ids"]
    labels = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], pad)], 1)
    labels = labels.masked_fill(labels == pad, -100)
    if caption_infer["text_feats"].is_cuda:
        caption_loss, logits, labels = _mlm_head(pl_module, caption_infer["text_feats"], labels)
    else:                                                    # host tests: the same cross entropy in torch
        logits = pl_module.mlm_score(caption_infer["text_feats"])
        caption_loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]).float(), labels.reshape(-1), ignore_index=-100)
    loss = alpha * caption_loss + (1 - alpha) * rl_loss
    ret = {"caption_cider_loss": loss, "caption_cider_logits": logits, "caption_cider_labels": labels, "caption_cider_ids": ids}
    phase = "train" if pl_module.training else "val"
    loss = getattr(pl_module, f"{phase}_caption_cider_loss")(ret["caption_cider_loss"])
    acc = getattr(pl_module, f"{phase}_caption_cider_accuracy")(ret["caption_cider_logits"], ret["caption_cider_labels"])
    pl_module.log(f"caption_cider/{phase}/loss", loss)
    pl_module.log(f"caption_cider/{phase}/accuracy", acc)
    return ret


@torch.no_grad()
def caption_test_step(pl_module, batch, output, beam_size=5):
    """objectives.py:560-645: beam search over max_text_len - 1 steps.  The image tokens are computed once (the first infer_caption,
    on the batch's own text) and repeated per beam; every step re-runs the whole causal text stack on the current ids
    (text_masks None) and scores one position, the [MASK] logit forced to -10000; candidates are ranked by length-normalised
    log-probability, and the search stops early once every beam has ended.  Returns the captions (tokenizer.decode of beam 0, sep /
    cls -> pad, pad removed) and, not in the reference, the ids beam 0 generated (sep kept, padding after it) under `caption_ids`
    ([B, max_text_len - 1]).

    config["caption_decode_cache"]: one image pass, then one token per beam and step through pl_module.caption_decoder (_cached_feats) with
    the beam reorder `top_prev` as its `parent`; the bookkeeping below is the same.  The same function up to bf16 rounding."""
    captions = []
    if pl_module.training:
        return {"image_ids": batch["iid"], "captions": captions, "caption_ids": None}
    tok = pl_module.trainer.datamodule.dms[0].tokenizer
    max_len = pl_module.hparams.config["max_text_len"]
    batch = dict(batch)                                   # (the reference overwrites text_ids / text_masks in the caller's batch)
    bs, dev = batch["text_ids"].size(0), batch["text_ids"].device
    text_ids = torch.full((bs, max_len), tok.pad_token_id, device=dev, dtype=batch["text_ids"].dtype)
    text_ids[:, 0] = tok.cls_token_id
    search = bs * beam_size
    end_seq = torch.zeros(bs, dtype=torch.bool, device=dev)
    cached = bool(pl_module.hparams.config.get("caption_decode_cache", False))
    if cached:
        feats_at = _cached_feats(pl_module, pl_module.caption_image_embeds(batch["image_0" if "image_0" in batch else "image"][0]), beam_size)
    else:
        first = pl_module.infer_caption(batch, mask_text=False, mask_image=False)
        image_embeds = first["image_embeds"]
        batch["text_masks"] = None

        def feats_at(i, ids, parent):
            batch["text_ids"] = ids
            infer = first if i == 0 else pl_module.infer_caption(batch, mask_text=False, mask_image=False, image_embeds=image_embeds)
            return infer["text_feats"][:, i:i + 1]
    parent = None
    for i in range(max_len - 1):
        logits = pl_module.mlm_score(feats_at(i, text_ids, parent)).float()
        logits[:, 0, tok.mask_token_id] = -10000
        logp = torch.log_softmax(logits, dim=-1)                                  # [N, 1, V]
        if i == 0:
            top = logp.argsort(descending=True, dim=-1)[:, :, :beam_size]         # [bs, 1, beam]
            head_logp = logp.gather(-1, top).view(search, 1)
            tgt = top.permute(0, 2, 1).reshape(search, 1)
            head_lengths = torch.ones_like(head_logp)
            text_ids = text_ids.view(bs, 1, -1).repeat(1, beam_size, 1).view(search, -1)
            padded = torch.full((search, 1), tok.pad_token_id, dtype=torch.long, device=dev)
            if not cached:
                hs = image_embeds.size(-1)
                image_embeds = image_embeds.view(bs, 1, -1, hs).repeat(1, beam_size, 1, 1).view(search, -1, hs)
        else:
            lengths = 1.0 - end_seq.to(logp.dtype)                                # ended beams add nothing
            logp = (logp * lengths[:, :, None] + head_logp[:, :, None]).view(bs, beam_size, 1, -1).permute(0, 2, 1, 3)
            V = logp.size(3)
            lengths = (lengths + head_lengths).view(bs, beam_size, 1).permute(0, 2, 1)
            normed = (logp / (lengths[:, :, :, None] + 1e-9)).contiguous().view(bs, 1, -1)
            top_idx = normed.argsort(descending=True, dim=-1)[:, :, :beam_size]
            top_logp = logp.contiguous().view(bs, 1, -1).gather(-1, top_idx)
            top_tokens = (top_idx % V).permute(0, 2, 1).contiguous().view(search, 1)
            top_prev = top_idx // V + torch.arange(bs, dtype=torch.long, device=dev)[:, None, None] * beam_size
            top_prev = top_prev.permute(0, 2, 1).contiguous().view(search, 1)
            head_logp = top_logp.permute(0, 2, 1).contiguous().view(search, 1)
            head_lengths = lengths.permute(0, 2, 1).contiguous().view(search, 1)  # (per beam slot, not gathered: as the reference)
            prev_ended = end_seq.gather(0, top_prev).to(torch.long)
            tgt = (1 - prev_ended) * top_tokens + prev_ended * padded
            text_ids = text_ids.gather(0, top_prev.repeat(1, text_ids.size(1)))
            parent = top_prev.view(-1)
        text_ids[:, i + 1] = tgt.view(-1)
        end_seq = (tgt == tok.sep_token_id) | (tgt == tok.pad_token_id)
        if i > 0 and bool(end_seq.all()):
            break
    gen = text_ids.view(bs, beam_size, -1)[:, 0, 1:].contiguous()
    ids = gen.clone()
    ids[ids == tok.sep_token_id] = tok.pad_token_id
    ids[ids == tok.cls_token_id] = tok.pad_token_id
    for t in ids:
        captions.append(tok.decode(t.tolist()).replace(tok.pad_token, ""))
    return {"image_ids": batch["iid"], "captions": captions, "caption_ids": gen}


def caption_test_wrapup(outs, model_name, out_dir="result"):
    """objectives.py:647-680: every rank writes its (image_id, caption) shard, rank 0 merges the shards (first caption per image id)
    into result/caption.json."""
    import glob
    import json
    import os
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if multi else 0
    records = [{"image_id": iid, "caption": c} for out in outs for iid, c in zip(out["image_ids"], out["captions"])]
    shard = f"caption_{rank}.json"
    with open(shard, "w") as fp:
        json.dump(records, fp, indent=4)
    if multi:
        dist.barrier()
    if rank == 0:
        merged, seen = [], set()
        for path in glob.glob("caption_*.json"):
            with open(path) as fp:
                for x in json.load(fp):
                    if x["image_id"] not in seen:
                        merged.append(x)
                        seen.add(x["image_id"])
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "caption.json"), "w") as fp:
            json.dump(merged, fp, indent=4)
    if multi:
        dist.barrier()
    os.remove(shard)


@torch.no_grad()
def init_weights(module):
    # in-place ops on the parameters themselves, not on `.data`: they bump the version counter, so the derived weight copies of
    # fiber_amd/ops.py see a re-initialisation after a forward pass (same values, same generator draws as the `.data` form)
    if isinstance(module, (nn.Linear, nn.Embedding)):
        module.weight.normal_(mean=0.0, std=0.02)
    elif isinstance(module, nn.LayerNorm):
        module.bias.zero_()
        module.weight.fill_(1.0)
    if isinstance(module, nn.Linear) and module.bias is not None:
        module.bias.zero_()
