"""Grounding head of the fine-grained model on the MI355X kernels: VLDyHead for the FIBER configuration + the token focal loss.

Mirrors fine_grained/maskrcnn_benchmark/modeling/rpn/vldyhead.py:587-915 (VLDyHead; its Conv3x3Norm :118-154 and DyConv :157-251) and
layers/sigmoid_focal_loss.py:130-195 (token_sigmoid_binary_focal_loss, TokenSigmoidFocalLoss) for what every FIBER fine-grained config
instantiates: FUSE_CONFIG.TYPE "NONE", EARLY_FUSE_ON False (the fusion happened in the backbone), USE_DOT_PRODUCT_TOKEN_LOSS True.
Constructor reads, parameter names and shapes are the reference's, hence the same checkpoint keys: `dyhead_tower.<i>.DyConv.<j>.conv.*`,
`...bn.*`, `...offset.*`, `...AttnConv.1.*`, `...relu.fc.*`, `cls_logits.*`, `bbox_pred.*`, `centerness.*`,
`dot_product_projection_text.{weight,bias}`, `log_scale`, `bias_lang`, `bias0`, `scales.<l>.scale`.

The tower is modules/dyhead.py's DyConv (deformable convolutions on csrc/dcn.hip) taking and returning the {"visual", "lang"} dict; the
region-word dot product and the loss are csrc/ground.hip through ops.ground_logits / ops.ground_token_loss.  The text side (F.normalize,
/2, the 768 -> 256 linear, embedding @ bias_lang + bias0: B x 256 rows) and the three 1x1 prediction convolutions (1 + 4 + 1 output
channels at num_anchors = 1) stay plain torch fp32 on the device: a few hundred KB, no kernels of their own.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from . import dyhead

_UNSUPPORTED = {
    "EARLY_FUSE_ON": "VLFuse / BertEncoderLayer in the tower: FIBER fuses in the backbone (FUSE_CONFIG.TYPE NONE)",
    "USE_TOKEN_LOSS": "the convolutional token head: FIBER uses the dot-product token loss",
    "USE_CONTRASTIVE_ALIGN_LOSS": "MDETR-style contrastive alignment: excluded by USE_DOT_PRODUCT_TOKEN_LOSS",
    "USE_SHALLOW_CONTRASTIVE_LOSS": "shallow contrastive loss on FPN features: never set by a FIBER config",
    "USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS": "shallow contrastive loss on backbone features: never set by a FIBER config",
    "MLM_LOSS": "BertLMPredictionHead on the head: never set by a FIBER config",
    "USE_FUSED_FEATURES_DOT_PRODUCT": "language features from the tower: needs EARLY_FUSE_ON",
}


class Scale(nn.Module):
    """layers/misc.py:101-107"""

    def __init__(self, init_value=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.FloatTensor([init_value]))

    def forward(self, input):
        return input * self.scale


class DyConv(dyhead.DyConv):
    """vldyhead.py:157-251: layers/dyhead.py's DyConv on the {"visual": [levels], "lang": ...} dict."""

    def forward(self, inputs):
        return {"visual": super().forward(inputs["visual"]), "lang": inputs["lang"]}


def permute_and_flatten(layer, N, A, C, H, W):
    """modeling/utils.py:19-23"""
    return layer.view(N, -1, C, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, C)


class TokenSigmoidFocalLoss(nn.Module):
    """layers/sigmoid_focal_loss.py:174-195 for callers that already hold logits [B, A, T] (version "binary", :130-171), in the stable
    form the kernel uses: ce = softplus(-z), 1 - p_t = sigmoid(-z), z = +logit for target 1 and -logit for target 0.  Plain torch: the
    training path is VLDyHead.token_loss, which never forms the logits."""

    def __init__(self, alpha, gamma):
        super().__init__()
        self.alpha, self.gamma = alpha, gamma

    def forward(self, logits, targets, text_masks=None, version="binary", **kwargs):
        if targets.nelement() == 0:
            return torch.as_tensor(0, device=logits.device)
        if version != "binary":
            raise NotImplementedError(f"TokenSigmoidFocalLoss version {version!r}: FIBER trains with \"binary\"")
        pos = targets != 0
        z = torch.where(pos, logits, -logits)
        loss = F.softplus(-z) * torch.exp(-self.gamma * F.softplus(z))
        if self.alpha >= 0:
            loss = loss * torch.where(pos, self.alpha, 1.0 - self.alpha).to(loss.dtype)
        if text_masks is not None:
            loss = loss * (text_masks > 0).unsqueeze(1).to(loss.dtype)
        return loss.sum()

    def __repr__(self):
        return f"{self.__class__.__name__}(gamma={self.gamma}, alpha={self.alpha})"


class VLDyHead(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        d, fc = cfg.MODEL.DYHEAD, cfg.MODEL.DYHEAD.FUSE_CONFIG
        if cfg.MODEL.LANGUAGE_BACKBONE.MODEL_TYPE not in ("bert-base-uncased", "roberta-base", "roberta-fused", "roberta-fused-v2", "clip"):
            raise NotImplementedError
        for key, why in _UNSUPPORTED.items():
            if getattr(fc, key, False):
                raise NotImplementedError(f"DYHEAD.FUSE_CONFIG.{key}: {why}")
        if not fc.USE_DOT_PRODUCT_TOKEN_LOSS:
            raise NotImplementedError("DYHEAD.FUSE_CONFIG.USE_DOT_PRODUCT_TOKEN_LOSS must be set: it is the only token head FIBER builds")
        if getattr(d, "CONV_FUNC", ""):
            raise NotImplementedError("DYHEAD.CONV_FUNC: evaluated conv factories are not used by a FIBER config")
        if not d.USE_GN and (getattr(d, "USE_NSYNCBN", False) or getattr(d, "USE_SYNCBN", False)):
            raise NotImplementedError("DYHEAD.USE_NSYNCBN / USE_SYNCBN: FIBER configs normalise the tower with GroupNorm")

        num_classes = d.NUM_CLASSES - 1
        num_anchors = len(cfg.MODEL.RPN.ASPECT_RATIOS) * cfg.MODEL.RPN.SCALES_PER_OCTAVE
        if num_anchors != 1:
            raise NotImplementedError("the dot product pairs ONE 256-channel anchor feature per position with the tokens (vldyhead.py:861-865)")
        in_channels, channels = cfg.MODEL.BACKBONE.OUT_CHANNELS, d.CHANNELS
        groups = cfg.MODEL.GROUP_NORM.NUM_GROUPS if d.USE_GN else None
        use_dyrelu, use_dyfuse, use_deform = d.USE_DYRELU, d.USE_DYFUSE, d.USE_DFCONV

        def conv_func(i, o, s, deformable):
            m = dyhead.Conv3x3Norm(i, o, s, deformable=deformable, use_gn=False)
            if groups is not None:
                m.bn = nn.GroupNorm(num_groups=groups, num_channels=o)
            return m

        tower = []
        for i in range(d.NUM_CONVS):
            first = i == 0
            same = in_channels == channels
            deform = (use_deform and same) if first else use_deform
            tower.append(DyConv(in_channels if first else channels, channels,
                                # (:624 builds every Conv3x3Norm with deformable=use_deform; a DyConv without the offset predictor could
                                # not call it, so the FIBER configs -- in_channels == channels -- are the only ones this differs for)
                                conv_func=lambda a, b, s, _d=deform: conv_func(a, b, s, _d),
                                use_dyrelu=(use_dyrelu and same) if first else use_dyrelu,
                                use_dyfuse=(use_dyfuse and same) if first else use_dyfuse,
                                use_deform=deform))
        self.add_module("dyhead_tower", nn.Sequential(*tower))

        self.cls_logits = nn.Conv2d(channels, num_anchors * num_classes, kernel_size=1)
        self.bbox_pred = nn.Conv2d(channels, num_anchors * 4, kernel_size=1)
        self.centerness = nn.Conv2d(channels, num_anchors * 1, kernel_size=1)
        bias_value = -math.log((1 - d.PRIOR_PROB) / d.PRIOR_PROB)

        self.dot_product_projection_image = nn.Identity()
        self.dot_product_projection_text = nn.Linear(cfg.MODEL.LANGUAGE_BACKBONE.LANG_DIM, num_anchors * channels, bias=True)
        self.log_scale = nn.Parameter(torch.Tensor([d.LOG_SCALE]), requires_grad=True)
        self.bias_lang = nn.Parameter(torch.zeros(cfg.MODEL.LANGUAGE_BACKBONE.LANG_DIM), requires_grad=True)
        self.bias0 = nn.Parameter(torch.Tensor([bias_value]), requires_grad=True)

        for m in (self.cls_logits, self.bbox_pred, self.centerness):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)
        self.scales = nn.ModuleList([Scale(init_value=1.0) for _ in range(5)])
        nn.init.constant_(self.cls_logits.bias, bias_value)

    # ---- text side (vldyhead.py:796-801): B x T rows, fp32 torch
    def _tokens(self, embedding):
        embedding = F.normalize(embedding.float(), p=2, dim=-1)
        proj = self.dot_product_projection_text(embedding / 2.0)
        bias = torch.matmul(embedding, self.bias_lang) + self.bias0
        return proj, bias

    def _clamped(self):
        if not getattr(self.cfg.MODEL.DYHEAD.FUSE_CONFIG, "CLAMP_DOT_PRODUCT", True):
            raise NotImplementedError("DYHEAD.FUSE_CONFIG.CLAMP_DOT_PRODUCT False: the kernel always clamps to +-50000 (every FIBER config sets it)")

    def forward(self, x, language_dict_features=None, embedding=None, swint_feature_c4=None):
        self._clamped()
        tower = self.dyhead_tower({"visual": x, "lang": language_dict_features})["visual"]
        proj, tbias = self._tokens(embedding)
        logits, bbox_reg, centerness, dot_product_logits = [], [], [], []
        fused = [] if self.cfg.MODEL.RPN.RETURN_FUSED_FEATURES else None
        for l, f in enumerate(tower):
            logits.append(self.cls_logits(f))
            bbox_reg.append(self.scales[l](self.bbox_pred(f)))
            centerness.append(self.centerness(f))
            if fused is not None:
                fused.append(f)
            B, C, H, W = f.shape
            q = permute_and_flatten(self.dot_product_projection_image(f), B, -1, C, H, W)
            dot_product_logits.append(ops.ground_logits(q, proj, tbias, self.log_scale))
        return logits, bbox_reg, centerness, None, None, None, dot_product_logits, None, None, fused

    def training_outputs(self, x, embedding):
        """What training needs from ONE run of the tower (grounding_train.ATSSLossComputation): the per-level cls_logits, bbox_reg and
        centerness, all levels' anchor features concatenated [B, sum HW, C], the projected tokens and the token bias.  The alignment
        logits are never materialised."""
        self._clamped()
        tower = self.dyhead_tower({"visual": x, "lang": None})["visual"]
        proj, tbias = self._tokens(embedding)
        logits = [self.cls_logits(f) for f in tower]
        bbox_reg = [self.scales[l](self.bbox_pred(f)) for l, f in enumerate(tower)]
        centerness = [self.centerness(f) for f in tower]
        q = torch.cat([permute_and_flatten(f, f.shape[0], -1, f.shape[1], f.shape[2], f.shape[3]) for f in tower], dim=1)
        return logits, bbox_reg, centerness, q, proj, tbias

    def token_loss(self, x, embedding, targets, text_masks, num_pos, alpha=None, gamma=None):
        """Training entry point (modeling/rpn/loss.py:1222-1226): tower -> all levels' anchors concatenated [B, sum HW, C] ->
        ops.ground_token_loss / num_pos.  targets [B, sum HW, T] in the level order of `x`; the logits are never materialised.
        alpha / gamma default to cfg.MODEL.FOCAL.LOSS_ALPHA / LOSS_GAMMA (loss.py:1107)."""
        self._clamped()
        focal = getattr(self.cfg.MODEL, "FOCAL", None)
        alpha = alpha if alpha is not None else (focal.LOSS_ALPHA if focal is not None else 0.25)
        gamma = gamma if gamma is not None else (focal.LOSS_GAMMA if focal is not None else 2.0)
        tower = self.dyhead_tower({"visual": x, "lang": None})["visual"]
        proj, tbias = self._tokens(embedding)
        q = torch.cat([permute_and_flatten(f, f.shape[0], -1, f.shape[1], f.shape[2], f.shape[3]) for f in tower], dim=1)
        return ops.ground_token_loss(q, proj, tbias, self.log_scale, targets, text_masks, alpha, gamma) / num_pos
