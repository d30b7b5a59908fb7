"""FPN neck of the fine-grained model on the MI355X kernels.

Mirrors fine_grained/maskrcnn_benchmark/modeling/backbone/fpn.py (FPN :7-137, LastLevelP6P7 :145-163), layers/dropblock.py:6-77
(DropBlock2D) and the wiring of modeling/backbone/__init__.py:151-197 (build_retinanet_swint_fpn_backbone) with
make_layers.conv_with_kaiming_uniform (:79-108): same constructor meaning, forward input (a list of NCHW stage maps, or the
`(maps, text)` tuple) and parameter names, hence the same checkpoint keys: `fpn_inner{2,3,4}.{weight,bias}`,
`fpn_layer{2,3,4}.{weight,bias}`, `top_blocks.p{6,7}.{weight,bias}`, all nn.Conv2d-shaped.

The wiring's quirks are kept: `in_channels_list = [0, C3, C4, C5]` skips stage 2, the zip of fpn.py:90-92 then never reaches the
stride-4 map, and the output is five levels at strides 8 ... 128; P6 is read from P5 because in == out channels (:157), the ReLU sits
in front of P7 only; in training the DropBlock mask goes to the two top-down levels' 3x3 convolutions while the UNDROPPED sum feeds the
next merge, and the top level is never dropped (:89).

Kernels: the 1x1 laterals are the NT GEMM on the [B H W, Cin] tokens as they lie (ops.conv1x1), the 3x3 and stride-2 convolutions the
channels-last gather + MFMA GEMM (ops.deform_conv without offsets), the top-down pathway -- nearest up-sampling, add, DropBlock mask and
its batch-wide normaliser -- csrc/fpn.hip (ops.dropblock_mask, ops.fpn_merge): no host generator, no host-to-device copy, nothing read on
the host.  Maps travel channels-last bf16 between them (forward_nhwc); forward converts at both ends, to the NCHW fp32 convention of
dyhead._nchw that DyHead / VLDyHeadModule take.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .dyhead import _Conv2dNHWC, _nchw, _nhwc

_UNSUPPORTED = {
    "USE_GN": "GroupNorm inside the FPN convolutions (conv_with_kaiming_uniform): no FIBER config sets it",
    "USE_RELU": "ReLU inside the FPN convolutions (conv_with_kaiming_uniform): no FIBER config sets it",
    "USE_DYRELU": "DYReLU inside the FPN convolutions: no FIBER config sets it",
    "USE_SPP": "SPPLayer in front of the top lateral (fpn.py:84-85): no FIBER config sets it",
    "USE_PAN": "the bottom-up PAN path (fpn.py:112-125): no FIBER config sets it",
    "USE_DYHEAD": "a DyHead inside the backbone Sequential (backbone/__init__.py:193-195): FIBER's tower lives in the rpn head",
    "RETURN_SWINT_FEATURE_BEFORE_FUSION": "swint_feature_c4 for the shallow contrastive loss: no FIBER config sets it",
}


def _kaiming(conv):
    nn.init.kaiming_uniform_(conv.weight, a=1)
    nn.init.constant_(conv.bias, 0)
    return conv


class _Conv1x1NHWC(nn.Conv2d):
    """nn.Conv2d(Cin, Cout, 1) (same parameters / keys) whose forward is a GEMM on the channels-last tokens."""

    def forward_nhwc(self, x):
        return ops.conv1x1(x, self.weight, self.bias)

    def forward(self, input):
        return _nchw(self.forward_nhwc(_nhwc(input)))


def conv_with_kaiming_uniform(use_gn=False, use_relu=False, use_dyrelu=False):
    """make_layers.py:79-108 for the plain configuration"""
    for key, on in (("USE_GN", use_gn), ("USE_RELU", use_relu), ("USE_DYRELU", use_dyrelu)):
        if on:
            raise NotImplementedError(f"FPN.{key}: {_UNSUPPORTED[key]}")

    def make_conv(in_channels, out_channels, kernel_size, stride=1, dilation=1):
        if dilation != 1 or kernel_size not in (1, 3):
            raise NotImplementedError("FPN builds 1x1 and 3x3 convolutions with dilation 1 (fpn.py:48-49)")
        if kernel_size == 1:
            return _kaiming(_Conv1x1NHWC(in_channels, out_channels, kernel_size=1))
        return _kaiming(_Conv2dNHWC(in_channels, out_channels, kernel_size=3, stride=stride, padding=1))
    return make_conv


class DropBlock2D(nn.Module):
    """layers/dropblock.py:6-77: x * block_mask * numel / block_mask.sum() in training, x otherwise.  forward takes NCHW (any float
    dtype) and returns NCHW fp32; forward_nhwc channels-last bf16.  seeds ([B, H, W], non-zero = block centre) replaces the draw."""

    def __init__(self, drop_prob, block_size):
        super().__init__()
        if block_size % 2 == 0:
            raise NotImplementedError("FPN.DROP_SIZE even: the mask kernel pools an odd block around its centre (the default is 3)")
        self.drop_prob, self.block_size = drop_prob, block_size

    def mask(self, B, H, W, device, seeds=None):
        return ops.dropblock_mask(B, H, W, self.drop_prob, self.block_size, device, seeds)

    def forward_nhwc(self, x, seeds=None):
        if not self.training or self.drop_prob == 0.0:
            return x
        B, H, W, _ = x.shape
        return ops.fpn_merge(x, None, *self.mask(B, H, W, x.device, seeds))[1]

    def forward(self, x, seeds=None):
        assert x.dim() == 4, "Expected input with 4 dimensions (bsize, channels, height, width)"
        if not self.training or self.drop_prob == 0.0:
            return x
        return _nchw(self.forward_nhwc(_nhwc(x), seeds))


class LastLevelP6P7(nn.Module):
    """fpn.py:145-163"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.p6 = _kaiming(_Conv2dNHWC(in_channels, out_channels, 3, 2, 1))
        self.p7 = _kaiming(_Conv2dNHWC(out_channels, out_channels, 3, 2, 1))
        self.use_P5 = in_channels == out_channels

    def forward_nhwc(self, c5, p5):
        p6 = self.p6.forward_nhwc(p5 if self.use_P5 else c5)
        return [p6, self.p7.forward_nhwc(F.relu(p6))]

    def forward(self, c5, p5):
        return [_nchw(t) for t in self.forward_nhwc(_nhwc(c5), _nhwc(p5))]


class FPN(nn.Module):
    """fpn.py:7-137.  forward(x): x a list of NCHW maps in increasing depth (one per entry of in_channels_list; an entry of 0 has no
    blocks and its map is never read), or the (maps, text) tuple of the VL backbones -> tuple of NCHW fp32 levels, highest resolution
    first (with a tuple input: (levels, text, None), as the reference)."""

    def __init__(self, in_channels_list, out_channels, conv_block, top_blocks=None, drop_block=None, use_spp=False, use_pan=False,
                 return_swint_feature_before_fusion=False):
        super().__init__()
        for key, on in (("USE_SPP", use_spp), ("USE_PAN", use_pan), ("RETURN_SWINT_FEATURE_BEFORE_FUSION", return_swint_feature_before_fusion)):
            if on:
                raise NotImplementedError(f"FPN.{key}: {_UNSUPPORTED[key]}")
        if top_blocks is not None and not isinstance(top_blocks, LastLevelP6P7):
            raise NotImplementedError("FPN top_blocks: LastLevelP6P7 (the RETINANET wiring) or None")
        self.inner_blocks, self.layer_blocks = [], []
        for idx, in_channels in enumerate(in_channels_list, 1):
            if in_channels == 0:
                continue
            self.add_module(f"fpn_inner{idx}", conv_block(in_channels, out_channels, 1))
            self.add_module(f"fpn_layer{idx}", conv_block(out_channels, out_channels, 3, 1))
            self.inner_blocks.append(f"fpn_inner{idx}")
            self.layer_blocks.append(f"fpn_layer{idx}")
        self.top_blocks = top_blocks
        self.drop_block = drop_block

    def forward_nhwc(self, x, seeds=None):
        """x: channels-last bf16 maps [B, H, W, C] (entries the zip never reaches may be None) -> list of channels-last bf16 levels.
        seeds: one [B, H, W] map per dropped level in the order they are drawn (coarsest first), instead of the draw."""
        last_inner = getattr(self, self.inner_blocks[-1]).forward_nhwc(x[-1])
        results = [getattr(self, self.layer_blocks[-1]).forward_nhwc(last_inner)]          # the top level is never dropped (:89)
        drop = self.drop_block is not None and self.training and self.drop_block.drop_prob != 0.0
        seeds = list(seeds) if seeds is not None else None
        for feature, inner_block, layer_block in zip(x[:-1][::-1], self.inner_blocks[:-1][::-1], self.layer_blocks[:-1][::-1]):
            lateral = getattr(self, inner_block).forward_nhwc(feature)
            B, H, W, _ = lateral.shape
            if drop:
                keep, kept = self.drop_block.mask(B, H, W, lateral.device, seeds.pop(0) if seeds is not None else None)
                last_inner, dropped = ops.fpn_merge(lateral, last_inner, keep, kept)
                results.insert(0, getattr(self, layer_block).forward_nhwc(dropped))
            else:
                last_inner, _ = ops.fpn_merge(lateral, last_inner)
                results.insert(0, getattr(self, layer_block).forward_nhwc(last_inner))
        if self.top_blocks is not None:
            results.extend(self.top_blocks.forward_nhwc(x[-1], results[-1]))
        return results

    def forward(self, x, seeds=None):
        text = None
        if type(x) is tuple:
            x, text = x[0], x[1]
        used = len(self.inner_blocks)                                                      # the zip reaches the last `used` maps only
        maps = [_nhwc(f) if i >= len(x) - used else None for i, f in enumerate(x)]
        results = tuple(_nchw(t) for t in self.forward_nhwc(maps, seeds))
        return (results, text, None) if text is not None else results


def build_swint_fpn(cfg):
    """The `fpn` half of build_retinanet_swint_fpn_backbone (backbone/__init__.py:175-192)."""
    f = cfg.MODEL.FPN
    for key in ("USE_DYHEAD", "USE_SPP", "USE_PAN", "RETURN_SWINT_FEATURE_BEFORE_FUSION", "USE_GN", "USE_RELU", "USE_DYRELU"):
        if getattr(f, key, False):
            raise NotImplementedError(f"FPN.{key}: {_UNSUPPORTED[key]}")
    stages = cfg.MODEL.SWINT.OUT_CHANNELS
    out_channels = cfg.MODEL.BACKBONE.OUT_CHANNELS
    return FPN(in_channels_list=[0, stages[-3], stages[-2], stages[-1]], out_channels=out_channels,
               conv_block=conv_with_kaiming_uniform(f.USE_GN, f.USE_RELU),
               top_blocks=LastLevelP6P7(out_channels, out_channels),
               drop_block=DropBlock2D(f.DROP_PROB, f.DROP_SIZE) if f.DROP_BLOCK else None,
               use_spp=f.USE_SPP, use_pan=f.USE_PAN, return_swint_feature_before_fusion=f.RETURN_SWINT_FEATURE_BEFORE_FUSION)
