"""Image-text retrieval evaluation: recall@1/5/10 in both directions by ITC features or by the ITM ranking score (reference
coarse_grained/fiber/modules/objectives.py:266-385 compute_itc_recall, :388-499 compute_itm_recall; fiber_utils.py:48-60 picks one by
`get_recall_metric_itc`).

What differs from the reference's loops:
  * The tally is ops.retrieval_ranks (csrc/retrieval.hip): the rank of the first matching candidate per query, two reductions per row
    or column, instead of six topk calls.  The recalls are hits / N correctly rounded to fp32, which for N < 2^24 is bit-equal to the
    reference's (ids == topk_ids).float().max(..)[0].mean() on the host.  Nothing is read back to the host.
  * The ITM grid (every image against every text) shares what does not depend on the pair: text prefixes are encoded once, an image's
    prefix once per image, and only the fusion blocks run per pair (FIBERTransformerSS.encode_image_prefix / encode_text_prefix /
    score_pairs).  shared_prefix=False keeps the reference's scheme, a full infer(img=image.repeat(..)) per (image, text batch).
  * Ranks exchange tensors with all_gather (feature or score rows and ids), not pickled lists over a side group.  Images are sharded as
    DistributedSampler(shuffle=False) shards them, its padding by the head of the list included: the reference counts those duplicates,
    so they are counted here.  Every rank holds all texts.

The datamodules are not part of this package: RetrievalData is what the reference pulls out of
`trainer.datamodule.dms[0].make_no_false_val_dset(...)` -- image batches and text batches with their image ids -- and is attached to the
module as `pl_module.retrieval_data`.
"""
import math

import torch

from .. import ops

KS = (1, 5, 10)
PAIR_BATCH = 256          # pairs per score_pairs call: the fastest of 64 / 128 / 256 at Swin-B 384^2 (profiles/retrieval_eval.md)


class RetrievalData:
    """image_batches: [(image tensor [b, 3, H, W], img_index list of b ids)], the validation images once each in dataset order;
    text_batches: [dict(text_ids [t, S], text_masks [t, S], text_labels [t, S], img_index list of t ids)], every caption."""

    def __init__(self, image_batches, text_batches):
        self.image_batches, self.text_batches = list(image_batches), list(text_batches)
        for img, ids in self.image_batches:
            if img.dim() != 4 or img.shape[0] != len(ids):
                raise ValueError(f"RetrievalData: image batch {tuple(img.shape)} with {len(ids)} ids")
        for b in self.text_batches:
            if b["text_ids"].shape != b["text_masks"].shape or b["text_ids"].shape[0] != len(b["img_index"]):
                raise ValueError(f"RetrievalData: text batch {tuple(b['text_ids'].shape)} / {tuple(b['text_masks'].shape)} with "
                                 f"{len(b['img_index'])} ids")

    @property
    def num_images(self):
        return sum(len(ids) for _, ids in self.image_batches)

    @property
    def num_texts(self):
        return sum(len(b["img_index"]) for b in self.text_batches)


def pack_retrieval_data(images, img_index, text_ids, text_masks, text_img_index, image_batch=1, text_batch=64):
    """RetrievalData from tensors: images [N, 3, H, W] with N ids, text_ids / text_masks [T, S] with T image ids; batches of image_batch
    images (the reference loads them one at a time) and text_batch captions (the reference's 64)."""
    img_index, text_img_index = [int(i) for i in img_index], [int(i) for i in text_img_index]
    ib = [(images[i:i + image_batch], img_index[i:i + image_batch]) for i in range(0, len(img_index), image_batch)]
    tb = [dict(text_ids=text_ids[i:i + text_batch], text_masks=text_masks[i:i + text_batch],
               text_labels=torch.full_like(text_ids[i:i + text_batch], -100), img_index=text_img_index[i:i + text_batch])
          for i in range(0, len(text_img_index), text_batch)]
    return RetrievalData(ib, tb)


def shard_indices(n, world, rank):
    """The indices DistributedSampler(dataset of n, num_replicas=world, rank=rank, shuffle=False) yields: padded to a multiple of world by
    repeating the head of the list, then every world-th from `rank`."""
    per = math.ceil(n / world)
    idx = list(range(n))
    pad = per * world - n
    if pad > 0:
        idx += idx[:pad] if pad <= n else (idx * math.ceil(pad / n))[:pad]
    return idx[rank:per * world:world]


def _world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def _gather_rows(t):
    """Rank-major concatenation of equally shaped tensors (row counts are equal by the sampler's padding)"""
    import torch.distributed as dist
    world, _ = _world()
    if world == 1:
        return t
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t.contiguous())
    return torch.cat(out, dim=0)


def _local_images(data, chunk):
    """This rank's shard of the images in chunks of at most `chunk`: yields (images [b, 3, H, W], ids)"""
    world, rank = _world()
    where = [(b, r) for b, (_, ids) in enumerate(data.image_batches) for r in range(len(ids))]
    mine = shard_indices(len(where), world, rank)
    for i in range(0, len(mine), chunk):
        part = [where[g] for g in mine[i:i + chunk]]
        imgs = torch.stack([data.image_batches[b][0][r] for b, r in part])
        yield imgs, [data.image_batches[b][1][r] for b, r in part]


def _text_ids(data):
    return [int(i) for b in data.text_batches for i in b["img_index"]]


def _recalls(scores, iids, tiids):
    """-> (ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10), 0-d fp32 tensors on the scores' device"""
    _, _, hits = ops.retrieval_ranks(scores, iids, tiids, KS)
    # hits / N rounded to fp32 once: the quotient is formed in fp64 (53 >= 2 * 24 + 2 bits: rounding it again to fp32 gives the correctly
    # rounded fp32 quotient), because the device's own fp32 division is not the correctly rounded one
    ir = (hits[0].double() / float(scores.shape[1])).float()
    tr = (hits[1].double() / float(scores.shape[0])).float()
    return tuple(ir.unbind(0)) + tuple(tr.unbind(0))


def _matmul(a, b):
    return ops.lib_matmul(a, b) if a.is_cuda else torch.matmul(a, b)


@torch.no_grad()
def itc_scores(pl_module, data, image_batch=8, features=None):
    """-> (scores fp32 [Ni, Nt], iids int32 [Ni], tiids int32 [Nt]) of compute_itc_recall: columns in ascending tiids order
    (objectives.py:353-355), rows rank-major over the image shards.  features: (image_fn(images) -> [b, D], text_fn(batch) -> [t, D])
    instead of the module's image-only / text-only passes."""
    dev = pl_module.device
    if features is None:
        def image_fn(img):
            return pl_module.infer({"image": [img]}, image_only=True)["cls_feats"]

        def text_fn(b):
            return pl_module.infer(b, text_only=True)["cls_feats"]
    else:
        image_fn, text_fn = features
    text_feats = torch.cat([text_fn({k: b[k].to(dev) for k in ("text_ids", "text_masks", "text_labels")}).float()
                            for b in data.text_batches])
    feats, iids = [], []
    for img, ids in _local_images(data, image_batch):
        feats.append(image_fn(img.to(dev)).float())
        iids += ids
    image_feats = _gather_rows(torch.cat(feats))
    iids = _gather_rows(torch.tensor(iids, dtype=torch.int32, device=dev))
    tiids, order = torch.tensor(_text_ids(data), dtype=torch.int32).sort(stable=True)
    text_feats = text_feats.index_select(0, order.to(dev))
    return _matmul(image_feats, text_feats.t().contiguous()), iids, tiids.to(dev)


@torch.no_grad()
def itm_scores(pl_module, data, pair_batch=PAIR_BATCH, shared_prefix=True, image_batch=8, scores=None):
    """-> (scores fp32 [Ni, Nt], iids int32 [Ni], tiids int32 [Nt]) of compute_itm_recall: columns in the text batches' order, rows
    rank-major over the image shards.  scores: fn(images [b, 3, H, W]) -> fp32 [b, Nt] instead of the module's pair scoring."""
    dev = pl_module.device
    texts = [{k: b[k].to(dev) for k in ("text_ids", "text_masks", "text_labels")} for b in data.text_batches]
    Nt = data.num_texts
    world, _ = _world()
    n_local = math.ceil(data.num_images / world)
    out = torch.empty((n_local, Nt), dtype=torch.float32, device=dev)
    iids, row = [], 0
    if scores is None and shared_prefix:
        pre = [pl_module.encode_text_prefix(b["text_ids"], b["text_masks"]) for b in texts]
        text_prefix, ext = torch.cat([p[0] for p in pre]), torch.cat([p[1] for p in pre])
        t_all = torch.arange(Nt, device=dev)
    for img, ids in _local_images(data, image_batch):
        img = img.to(dev)
        n = img.shape[0]
        block = out[row:row + n]
        if scores is not None:
            block.copy_(scores(img))
        elif shared_prefix:
            image_prefix = pl_module.encode_image_prefix(img)
            flat = block.view(-1)                            # pair p of the chunk = (image p // Nt, text p % Nt): the rows of `out` in place
            i_idx, t_idx = torch.arange(n, device=dev).repeat_interleave(Nt), t_all.repeat(n)
            for p in range(0, n * Nt, pair_batch):
                flat[p:p + pair_batch] = pl_module.score_pairs(image_prefix, text_prefix, ext, i_idx[p:p + pair_batch],
                                                               t_idx[p:p + pair_batch])
        else:                                                # objectives.py:442-462
            for r in range(n):
                col = 0
                for b in texts:
                    t = b["text_ids"].shape[0]
                    cls = pl_module.infer(b, img=img[r:r + 1].repeat(t, 1, 1, 1))["cls_feats"]
                    block[r, col:col + t] = pl_module.rank_score(cls)
                    col += t
        iids += ids
        row += n
    iids = _gather_rows(torch.tensor(iids, dtype=torch.int32, device=dev))
    return _gather_rows(out), iids, torch.tensor(_text_ids(data), dtype=torch.int32, device=dev)


def compute_itc_recall(pl_module, data, image_batch=8, features=None):
    """objectives.py:266-385 -> (ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10), 0-d fp32 tensors"""
    return _recalls(*itc_scores(pl_module, data, image_batch, features))


def compute_itm_recall(pl_module, data, pair_batch=PAIR_BATCH, shared_prefix=True, image_batch=8, scores=None):
    """objectives.py:388-499 -> (ir_r1, ir_r5, ir_r10, tr_r1, tr_r5, tr_r10), 0-d fp32 tensors"""
    return _recalls(*itm_scores(pl_module, data, pair_batch, shared_prefix, image_batch, scores))


def evaluate_retrieval(pl_module, data, features=None, scores=None):
    """fiber_utils.py:49-52: ITC recall when config["get_recall_metric_itc"], else ITM recall"""
    if pl_module.hparams.config["get_recall_metric_itc"]:
        return compute_itc_recall(pl_module, data, features=features)
    return compute_itm_recall(pl_module, data, scores=scores)
