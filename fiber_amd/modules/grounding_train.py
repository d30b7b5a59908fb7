"""Grounding training of the fine-grained model on the MI355X kernels: targets -> ATSS assignment -> the reference's loss dict.

Mirrors fine_grained/maskrcnn_benchmark/modeling/rpn/loss.py:479-1264 (ATSSLossComputation: prepare_targets, GIoULoss,
compute_centerness_targets, __call__) and vldyhead.py:1069-1095 (the loss dict) for what every FIBER fine-grained config sets: one anchor per
location, ATSS.TOPK candidates per level, USE_DOT_PRODUCT_TOKEN_LOSS True, USE_CLASSIFICATION_LOSS False, RPN_ONLY True.

The reference loops over images with topk, boolean gathers, nonzero and .item() calls on [A, G] matrices: device-to-host synchronisations
in the middle of a training step.  Here targets travel as fixed-shape device tensors (GroundingTargets) and
  ops.atss_assign       candidates -> threshold + positives -> multi-gt resolution -> matched / labels / reg / token targets / num_pos
  ops.atss_box_losses   sum w (1 - giou), sum w, sum BCE(centerness, w) with bbox_reg / centerness read in place      (csrc/atss.hip)
  ops.ground_token_loss the region-word focal loss on the assignment's token targets                                 (csrc/ground.hip)
are composed without reading anything on the host: the normalisers are device tensors (all-reduced when a process group is initialised)
and the zero-positive case is a torch.where.

Deviations from the reference, each pinned by the atss_ties case of tests/atss_cases.py:
  * equal centre distances across a top-k cut go to the lowest anchor index (the reference's topk order on ties is unspecified);
  * an anchor positive for several gts of equal IoU goes to the lowest gt index (the reference's max(dim=1) on a CPU does the same).
reg_targets of unassigned anchors are 0 (the reference encodes gt 0 there and never reads it).
"""
import torch

from .. import ops

T = 256


class GroundingTargets:
    """boxes fp32 [B, Gmax, 4] (xyxy), labels int32 [B, Gmax], num_gt int32 [B], positive_map uint8 [B, Gmax, 256].  Rows
    g >= num_gt[b] are padding and are never read for a decision."""

    def __init__(self, boxes, labels, num_gt, positive_map):
        self.boxes, self.labels, self.num_gt, self.positive_map = boxes, labels, num_gt, positive_map

    def to(self, device):
        return GroundingTargets(self.boxes.to(device), self.labels.to(device), self.num_gt.to(device), self.positive_map.to(device))

    def unpack(self):
        """-> (per-image boxes, per-image labels, positive-map rows [sum G_b, 256]): pack_targets' input.  Synchronises (reads num_gt)."""
        n = self.num_gt.cpu().tolist()
        return ([self.boxes[b, :k] for b, k in enumerate(n)], [self.labels[b, :k] for b, k in enumerate(n)],
                torch.cat([self.positive_map[b, :k] for b, k in enumerate(n)], dim=0))


def pack_targets(per_image_boxes, per_image_labels, positive_map_rows, gmax=None, device=None):
    """The reference's per-image form -- a list of [G_b, 4] boxes and [G_b] labels, and the [sum G_b, 256] positive map in image order as
    prepare_targets slices it (loss.py:646-648) -- -> GroundingTargets, built on the host.  gmax: the fixed Gmax (default: the largest
    G_b, at least 1); padding rows are zero."""
    B = len(per_image_boxes)
    counts = [int(b.shape[0]) for b in per_image_boxes]
    if len(per_image_labels) != B or any(int(l.shape[0]) != n for l, n in zip(per_image_labels, counts)):
        raise ValueError("pack_targets: one label per box")
    rows = torch.as_tensor(positive_map_rows)
    if rows.dim() != 2 or rows.shape[0] != sum(counts) or rows.shape[1] != T:
        raise ValueError(f"pack_targets: positive map {tuple(rows.shape)} for {sum(counts)} boxes and {T} tokens")
    G = max(max(counts, default=0), 1) if gmax is None else int(gmax)
    if G < max(counts, default=0):
        raise ValueError(f"pack_targets: gmax {G} below the largest image's {max(counts)} boxes")
    boxes = torch.zeros((B, G, 4), dtype=torch.float32)
    labels = torch.zeros((B, G), dtype=torch.int32)
    pmap = torch.zeros((B, G, T), dtype=torch.uint8)
    off = 0
    for b, n in enumerate(counts):
        if n:
            boxes[b, :n] = torch.as_tensor(per_image_boxes[b]).reshape(n, 4).float().cpu()
            labels[b, :n] = torch.as_tensor(per_image_labels[b]).to(torch.int32).cpu()
            pmap[b, :n] = (rows[off:off + n] != 0).to(torch.uint8).cpu()
        off += n
    out = GroundingTargets(boxes, labels, torch.tensor(counts, dtype=torch.int32), pmap)
    return out.to(device) if device is not None else out


def normalisers(num_pos, sum_ctr):
    """loss.py:1196-1198, :1245 on device tensors: (max(all_reduce(sum num_pos) / world, 1), all_reduce(sum w) / world), through
    torch.distributed when a process group is initialised and plain otherwise.  Nothing is read on the host."""
    n = num_pos.sum().to(torch.float32).reshape(1)
    s = sum_ctr.detach().to(torch.float32).reshape(1)
    world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size()
        if world > 1:
            both = torch.cat([n, s])
            torch.distributed.all_reduce(both)
            n, s = both[:1], both[1:]
    return (n / float(world)).clamp_min(1.0).reshape(()), (s / float(world)).reshape(())


class ATSSLossComputation:
    """loss.py:479-1264 for the FIBER configuration.  __call__ -> (loss_cls, loss_reg, loss_centerness, loss_dot_product_token)."""

    def __init__(self, cfg):
        m = cfg.MODEL
        fc = m.DYHEAD.FUSE_CONFIG
        if getattr(fc, "USE_CLASSIFICATION_LOSS", False):
            raise NotImplementedError("DYHEAD.FUSE_CONFIG.USE_CLASSIFICATION_LOSS: the classification focal loss is not built "
                                      "(every FIBER config trains the dot-product token loss instead)")
        if not getattr(m, "RPN_ONLY", True):
            raise NotImplementedError("MODEL.RPN_ONLY False: box_selector_train and the ROI heads are not built (every FIBER config sets it)")
        if not fc.USE_DOT_PRODUCT_TOKEN_LOSS:
            raise NotImplementedError("DYHEAD.FUSE_CONFIG.USE_DOT_PRODUCT_TOKEN_LOSS must be set: it is the only token head FIBER builds")
        for key in ("USE_TOKEN_LOSS", "USE_CONTRASTIVE_ALIGN_LOSS", "USE_SHALLOW_CONTRASTIVE_LOSS", "USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS",
                    "MLM_LOSS"):
            if getattr(fc, key, False):
                raise NotImplementedError(f"DYHEAD.FUSE_CONFIG.{key}: never set by a FIBER config")
        if len(m.RPN.ASPECT_RATIOS) * m.RPN.SCALES_PER_OCTAVE != 1:
            raise NotImplementedError("RPN.ASPECT_RATIOS / SCALES_PER_OCTAVE: one anchor per location (every FIBER config)")
        atss = getattr(m, "ATSS", None)
        self.topk = int(getattr(atss, "TOPK", 9))
        self.reg_loss_weight = float(getattr(atss, "REG_LOSS_WEIGHT", 2.0))
        focal = getattr(m, "FOCAL", None)
        self.token_alpha = float(getattr(fc, "TOKEN_ALPHA", focal.LOSS_ALPHA if focal is not None else 0.25))
        self.token_gamma = float(getattr(fc, "TOKEN_GAMMA", focal.LOSS_GAMMA if focal is not None else 2.0))

    def box_losses(self, box_regression, centerness, anchors, assign):
        """-> (loss_reg, loss_centerness, num_pos_avg) of an ops.atss_assign result (loss.py:1194-1198, :1237-1258)"""
        giou, sum_ctr, bce = ops.atss_box_losses(box_regression, centerness, anchors, assign)
        num_pos_avg, sum_ctr_avg = normalisers(assign.num_pos, sum_ctr)
        has = assign.num_pos.sum() > 0                          # this rank's own positives (loss.py:1242), never read on the host
        zero = torch.zeros((), dtype=torch.float32, device=giou.device)
        loss_reg = torch.where(has, giou / torch.where(has, sum_ctr_avg, zero + 1.0), zero) * self.reg_loss_weight
        return loss_reg, torch.where(has, bce / num_pos_avg, zero), num_pos_avg

    def __call__(self, box_cls, box_regression, centerness, targets, anchors, features, proj_tokens, token_bias, log_scale, text_masks=None):
        """box_cls / box_regression / centerness: per level, as the head's convolutions return them; targets: GroundingTargets on the
        device; anchors: one [A_l, 4] tensor per level; features [B, sum HW, 256], proj_tokens [B, 256, 256], token_bias [B, 256]:
        VLDyHead.training_outputs."""
        assign = ops.atss_assign(anchors, targets, self.topk)
        loss_reg, loss_centerness, num_pos_avg = self.box_losses(box_regression, centerness, anchors, assign)
        token = ops.ground_token_loss(features, proj_tokens, token_bias, log_scale, assign.token_targets, text_masks, self.token_alpha,
                                      self.token_gamma) / num_pos_avg
        loss_cls = 0.0 * sum(c.float().sum() for c in box_cls)  # keeps cls_logits.* in the graph with zero gradients (vldyhead.py:1084)
        return loss_cls, loss_reg, loss_centerness, token
