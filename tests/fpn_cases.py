"""Case table of the FPN top-down kernels (csrc/fpn.hip) and of the neck built on them (fiber_amd/modules/fpn.py): shapes, seeded inputs,
the fp64 restatement and the per-element bounds.  Shared by tests/test_hip_fpn.py (the kernels against fp64, the module against the
reference-run fixtures tests/golden/fpn_*.npz), tests/test_fpn_compare_host.py (the restatement against the fixtures, the bounds against
mutations) and tools/gen_fpn_golden.py (which takes its inputs from here).  Nothing here needs a GPU to import.

The operations, channels-last (lateral [B, H, W, C], coarse [B, Hc, Wc, C], keep uint8 [B, H, W], kept = sum keep):
  src(dst)  = min(int(floor(float32(dst) * (float32(Hc) / float32(H)))), Hc - 1)     the ABI's nearest rule, the scale formed in fp32
  seeds[i]  = hash_u32(seed, i) < uint32(float32(gamma) * 2^32)                        (draw) i the flat index
  keep      = 1 - maxpool_{block x block, stride 1, pad block // 2}(seeds)
  s         = lateral + coarse[src];  inner = bf16(s);  dropped = bf16(s * keep * scale),  scale = B H W / kept
  g         = d_inner + d_dropped * keep * scale;  d_lateral = bf16(g);  d_coarse[hc, wc] = bf16(sum of g over the children of (hc, wc))
Indices are formed with numpy.float32 exactly as the kernels form them and everything after them in fp64, so every element of every
output is compared.

Bounds, |got - ref| <= bf16_store(ref) + CONST 2^-24 sum |terms|   (bf16_store: dcn_cases.py, half an ulp of bf16 at ref):
  inner      1 fp32 operation (the add),                                   terms |lateral| + |coarse|
  dropped    4 (the add, the divide of the scale, two multiplies),         terms (|lateral| + |coarse|) keep scale
  d_lateral  4 (the divide, two multiplies, the add),                      terms |d_inner| + |d_dropped| keep scale
  d_coarse   n_children + 2 (the above without the exact first add, then the n - 1 adds of the children), terms sum over the children
CONST is twice the operation count: its ceiling, in the manner of dcn_cases.ceilings()."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from dcn_cases import bf16_store
from oracle import detgen
from oracle.image_ref import hash_u32

F32 = 2.0 ** -24
NAN_BF16 = -32768 + 0x7FC0    # bf16 quiet NaN 0xFFC0 as int16
GUARD = 64                    # guard elements after every output
OPS = {"inner": 1, "dropped": 4, "d_lateral": 4}              # d_coarse: n_children + 2 per element


def const(n_ops):
    return 2.0 * n_ops


# ---- kernel cases ---------------------------------------------------------------------------------------------------------------------
# name: (B, H, W, Hc, Wc, C) -- the smallest shapes at which the merge kernels can go wrong
MERGE_CASES = {
    "odd_2_4": (1, 5, 6, 3, 3, 8),              # odd sizes; coarse pixels with 2 and 4 children
    "odd_1_2_4": (1, 5, 5, 3, 3, 8),            # ... and with 1, 2 and 4 (rows 0, 0, 1, 1, 2 in both directions)
    "f32_rule": (1, 58, 8, 30, 4, 8),           # the fp32 index rule: the exact rational differs at (58, 30)
    "same_size": (1, 7, 9, 7, 9, 16),           # fpn.py:100-101
    "sixteen": (1, 4, 4, 1, 1, 8),              # 16 children
    "vec_tail": (2, 13, 17, 7, 9, 520),         # a vector tail beyond a power of two, two images, more than one workgroup
}
MASK_SHAPES = ((1, 1, 1), (2, 2, 3), (2, 25, 33))
MASK_BLOCKS = (1, 3, 5)
MASK_SEED = 0x5EED00000000 + 17
DROP_PROB, DROP_SIZE = 0.3, 3                   # MODEL.FPN.DROP_PROB / DROP_SIZE defaults


def src_index(n_dst, n_src):
    """The ABI's nearest rule for every dst, in fp32 as the kernels and upsample_nearest2d (size= given) evaluate it"""
    scale = np.float32(n_src) / np.float32(n_dst)
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float32) * scale).astype(np.int64), n_src - 1)


def src_index_integer(n_dst, n_src):
    """MUTATION: the exact rational dst * n_src // n_dst (what an integer-arithmetic kernel would compute)"""
    return np.minimum(np.arange(n_dst, dtype=np.int64) * n_src // n_dst, n_src - 1)


def hash_seeds(seed, shape, gamma):
    thresh = int(float(np.float32(gamma)) * 4294967296.0)
    n = int(np.prod(shape))
    return np.array([1 if hash_u32(seed, i) < thresh else 0 for i in range(n)], dtype=np.uint8).reshape(shape)


def mask_ref(seeds, block):
    """-> (keep uint8 [B, H, W], kept int) of seeds uint8 [B, H, W]: dropblock.py:61-74 written out on integers"""
    B, H, W = seeds.shape
    half = block // 2
    pad = np.zeros((B, H + 2 * half, W + 2 * half), dtype=np.uint8)
    pad[:, half:half + H, half:half + W] = seeds != 0
    pooled = np.zeros((B, H, W), dtype=np.uint8)
    for dy in range(block):
        for dx in range(block):
            pooled |= pad[:, dy:dy + H, dx:dx + W]
    keep = (1 - pooled).astype(np.uint8)
    return keep, int(keep.sum())


def _bf16_exact(a):
    return torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).double().numpy()


def merge_inputs(name, with_keep):
    """Seeded bf16-exact inputs of a merge case (fp64 numpy): lateral, coarse, d_inner, d_dropped and -- with_keep -- keep / kept from
    Bernoulli(0.08) block centres pooled with block 3"""
    B, H, W, Hc, Wc, C = MERGE_CASES[name]
    g = detgen._rng("fpn:merge:" + name, 0)
    x = dict(lateral=_bf16_exact(g.standard_normal((B, H, W, C))), coarse=_bf16_exact(g.standard_normal((B, Hc, Wc, C))),
             d_inner=_bf16_exact(g.standard_normal((B, H, W, C))), d_dropped=_bf16_exact(g.standard_normal((B, H, W, C))))
    if with_keep:
        seeds = (g.random((B, H, W)) < 0.08).astype(np.uint8)
        x["keep"], x["kept"] = mask_ref(seeds, 3)
        if x["kept"] == 0:                                      # (a one-pixel map: keep it non-degenerate, kept == 0 is documented only)
            x["keep"] = np.ones((B, H, W), dtype=np.uint8)
            x["kept"] = B * H * W
    return x


def merge_fwd_ref(x, index=src_index, scale_from_rounded=False):
    """fp64 forward -> {name: (ref, bound)} for inner and (when x has keep) dropped.  index / scale_from_rounded: the mutations."""
    lat, co = x["lateral"], x["coarse"]
    B, H, W, C = lat.shape
    ih, iw = index(H, co.shape[1]), index(W, co.shape[2])
    up = co[:, ih][:, :, iw]
    s = lat + up
    mag = np.abs(lat) + np.abs(up)
    out = {"inner": (s, bf16_store(s) + const(OPS["inner"]) * F32 * mag)}
    if "keep" in x:
        k = x["keep"][..., None].astype(np.float64)
        scale = float(B * H * W) / float(x["kept"])
        base = torch.from_numpy(s).to(torch.bfloat16).double().numpy() if scale_from_rounded else s
        d = base * k * scale
        out["dropped"] = (d, bf16_store(d) + const(OPS["dropped"]) * F32 * mag * k * scale)
    return out


def merge_bwd_ref(x, use_inner=True, use_dropped=True, index=src_index):
    """fp64 backward -> {name: (ref, bound)} for d_lateral and d_coarse"""
    B, H, W, C = x["lateral"].shape
    Hc, Wc = x["coarse"].shape[1:3]
    g = np.zeros((B, H, W, C))
    mag = np.zeros((B, H, W, C))
    if use_inner:
        g += x["d_inner"]
        mag += np.abs(x["d_inner"])
    if use_dropped:
        k = x["keep"][..., None].astype(np.float64)
        scale = float(B * H * W) / float(x["kept"])
        g += x["d_dropped"] * k * scale
        mag += np.abs(x["d_dropped"]) * k * scale
    ih, iw = index(H, Hc), index(W, Wc)
    dc, dmag, n = np.zeros((B, Hc, Wc, C)), np.zeros((B, Hc, Wc, C)), np.zeros((Hc, Wc))
    for h in range(H):
        for w in range(W):
            dc[:, ih[h], iw[w]] += g[:, h, w]
            dmag[:, ih[h], iw[w]] += mag[:, h, w]
            n[ih[h], iw[w]] += 1
    return {"d_lateral": (g, bf16_store(g) + const(OPS["d_lateral"]) * F32 * mag),
            "d_coarse": (dc, bf16_store(dc) + const(1) * (n[None, :, :, None] + 2) * F32 * dmag)}


# ---- the neck: the fixture's geometry, inputs and restatement ----------------------------------------------------------------------------
NECK = dict(B=2, stage_channels=(32, 64, 128), out_channels=16, stage2=(16, 50, 66), sizes=((25, 33), (13, 17), (7, 9)))
LEVEL_SIZES = ((25, 33), (13, 17), (7, 9), (4, 5), (2, 3))
OUT_NAMES = ("p3", "p4", "p5", "p6", "p7")
GOLDEN = "fpn_neck"
DRAW_SEED = 1234                                # torch.manual_seed before the reference's train-mode forward
WEIGHT_KEYS = tuple(f"fpn_{kind}{i}.{p}" for i in (2, 3, 4) for kind in ("inner", "layer") for p in ("weight", "bias")) + \
    tuple(f"top_blocks.p{i}.{p}" for i in (6, 7) for p in ("weight", "bias"))


def neck_inputs():
    """The four stage maps (NCHW fp32, bf16-exact; the first is the stride-4 map the wiring never reads) and the five projections of the
    linear loss sum_l <out_l, proj_l>"""
    g = detgen._rng("fpn:neck", 0)
    r = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32)).to(torch.bfloat16).float()   # noqa: E731
    B = NECK["B"]
    maps = [r(B, NECK["stage2"][0], *NECK["stage2"][1:])] + [r(B, c, h, w) for c, (h, w) in zip(NECK["stage_channels"], NECK["sizes"])]
    proj = [r(B, NECK["out_channels"], h, w) for h, w in LEVEL_SIZES]
    return maps, proj


def neck_cfg(**fpn):
    """The configuration nodes build_swint_fpn reads"""
    ns = types.SimpleNamespace
    f = dict(USE_GN=False, USE_RELU=False, USE_DYRELU=False, USE_SPP=False, USE_PAN=False, USE_DYHEAD=False,
             RETURN_SWINT_FEATURE_BEFORE_FUSION=False, DROP_BLOCK=True, DROP_PROB=DROP_PROB, DROP_SIZE=DROP_SIZE, FREEZE=False)
    f.update(fpn)
    return ns(MODEL=ns(SWINT=ns(OUT_CHANNELS=(16,) + NECK["stage_channels"]), BACKBONE=ns(OUT_CHANNELS=NECK["out_channels"]), FPN=ns(**f)))


class _Round(torch.autograd.Function):
    """A bf16 store: the value going forward and the gradient coming back are rounded to bf16"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def neck_ref(weights, maps, train_seeds=None, bf16=False, mutate=None):
    """fp64 restatement of the RETINANET wiring of fpn.py on NCHW maps -> the five levels.  weights: {key: tensor}; maps: the four stage
    maps; train_seeds: [stride-16 draw, stride-8 draw] ([B, H, W], non-zero = block centre) for the training-mode forward, None for eval.
    bf16: round the operands of every convolution and every stored map to bf16 where the product does (fp64 accumulation in between).
    mutate: "drop_top" (the top level dropped as well, by one block centre in its corner), "p6_from_c5" (P6 read from C5's lateral, the only C5-derived map of P6's input width), "int_index" (the exact-rational nearest
    rule)."""
    rd = _Round.apply if bf16 else (lambda t: t)
    rd_w = (lambda t: t + (t.to(torch.bfloat16).to(t.dtype) - t).detach()) if bf16 else (lambda t: t)     # the bf16 working copy; dW stays fp32
    w = {k: v.double() for k, v in weights.items()}

    def conv(x, name, stride=1):
        wt = w[name + ".weight"]
        return rd(F.conv2d(rd(x), rd_w(wt), w[name + ".bias"], stride=stride, padding=wt.shape[-1] // 2))

    def drop(s, seeds):
        keep, kept = mask_ref(np.asarray(seeds), DROP_SIZE)
        k = torch.from_numpy(keep).double()[:, None]
        return s * k * (float(keep.size) / float(kept))

    index = src_index_integer if mutate == "int_index" else src_index
    x = [m.double() for m in maps]
    last_inner = conv(x[3], "fpn_inner4")
    top = last_inner
    if mutate == "drop_top" and train_seeds is not None:
        corner = np.zeros((last_inner.shape[0],) + tuple(last_inner.shape[2:]), dtype=np.uint8)
        corner[:, 0, 0] = 1
        top = rd(drop(last_inner, corner))
    results = [conv(top, "fpn_layer4")]
    seeds = list(train_seeds) if train_seeds is not None else None
    for feature, i in ((x[2], 3), (x[1], 2)):
        lateral = conv(feature, f"fpn_inner{i}")
        H, W = lateral.shape[-2:]
        ih = torch.from_numpy(index(H, last_inner.shape[2]))
        iw = torch.from_numpy(index(W, last_inner.shape[3]))
        s = lateral + last_inner[:, :, ih][:, :, :, iw]
        last_inner = rd(s)
        results.insert(0, conv(rd(drop(s, seeds.pop(0))) if seeds is not None else last_inner, f"fpn_layer{i}"))
    p6 = conv(conv(x[3], "fpn_inner4") if mutate == "p6_from_c5" else results[-1], "top_blocks.p6", 2)
    p7 = conv(F.relu(p6), "top_blocks.p7", 2)
    return results + [p6, p7]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-300))


# rel-L2 distance of neck_ref(bf16=True) from the reference-run fixture, per output (tools/gen_fpn_golden.py prints them; the test
# test_fpn_compare_host.py::test_bf16_restatement_distances_are_the_recorded_ones pins them).  The GPU is allowed twice these: the
# factor 2 covers the fp32 accumulation order of the MFMA GEMMs, which the restatement (fp64 accumulation) does not model.
BF16_DISTANCE = {
    'eval.p3': 0.004044, 'eval.p4': 0.003708, 'eval.p5': 0.003368,
    'eval.p6': 0.004188, 'eval.p7': 0.004123, 'train.p3': 0.00397,
    'train.p4': 0.003682, 'train.p5': 0.003368, 'train.p6': 0.004188,
    'train.p7': 0.004123, 'grad.x3': 0.003778, 'grad.x4': 0.003912,
    'grad.x5': 0.004126, 'grad.fpn_inner2.weight': 0.002979, 'grad.fpn_inner2.bias': 0.003128,
    'grad.fpn_layer2.weight': 0.003284, 'grad.fpn_layer2.bias': 2.229e-08, 'grad.fpn_inner3.weight': 0.003263,
    'grad.fpn_inner3.bias': 0.003383, 'grad.fpn_layer3.weight': 0.002979, 'grad.fpn_layer3.bias': 0.0,
    'grad.fpn_inner4.weight': 0.003355, 'grad.fpn_inner4.bias': 0.003468, 'grad.fpn_layer4.weight': 0.00329,
    'grad.fpn_layer4.bias': 0.003991, 'grad.top_blocks.p6.weight': 0.003797, 'grad.top_blocks.p6.bias': 0.001621,
    'grad.top_blocks.p7.weight': 0.00377, 'grad.top_blocks.p7.bias': 0.0,
}
GPU_FACTOR = 2.0
# The gradients of fpn_layer2.bias, fpn_layer3.bias and top_blocks.p7.bias are plain sums of the (bf16-exact) projection: no bf16 rounding
# enters them, the restatement's distance is the reference's own fp32 summation error (or 0), and twice that would ask an fp32 sum in
# another order to be bit-exact.  For a bias gradient the tolerance is therefore never below the first-order bound of an fp32 sum of
# its n = B H W terms, (n - 1) 2^-24 sum |t| per channel, taken as rel-L2 over the channels (sum_floor).


def sum_floor(terms):
    """terms [B, C, H, W]: the summands of a per-channel sum -> rel-L2 of the worst-case fp32 summation error over the channels"""
    t = torch.as_tensor(terms).double()
    n = t.shape[0] * t.shape[2] * t.shape[3]
    err = (n - 1) * F32 * t.abs().sum(dim=(0, 2, 3))
    return float(err.norm() / t.sum(dim=(0, 2, 3)).norm())


def gpu_tolerance(name, floor=0.0):
    return max(GPU_FACTOR * BF16_DISTANCE[name], floor)


# ---- the end-to-end model's configuration ---------------------------------------------------------------------------------------------
def model_cfg(depths=(2, 2, 2, 2), convs=2, **over):
    """A FIBER fine-grained configuration at Swin-B / RoBERTa-base widths (the fused backbone hard-wires them) with a shallow Swin and a
    short tower: the nodes GeneralizedVLRCNN, build_swint_fpn, VLDyHeadModule and ATSSLossComputation read."""
    import ground_cases as gc
    ns = types.SimpleNamespace
    cfg = gc.head_cfg(convs=convs)
    m = cfg.MODEL
    m.SWINT = ns(VERSION="fusion", EMBED_DIM=128, DEPTHS=depths, NUM_HEADS=(4, 8, 16, 32), WINDOW_SIZE=12, MLP_RATIO=4.0, DROP_PATH_RATE=0.0,
                 APE=False, OUT_CHANNELS=(128, 256, 512, 1024))
    m.BACKBONE = ns(CONV_BODY="SWINT-FPN-RETINANET", FUSION_VERSION="v2", OUT_CHANNELS=256, FREEZE=False)
    m.FPN = neck_cfg().MODEL.FPN
    m.RPN = ns(ASPECT_RATIOS=(1.0,), SCALES_PER_OCTAVE=1, RETURN_FUSED_FEATURES=False, ANCHOR_SIZES=(64, 128, 256, 512, 1024),
               ANCHOR_STRIDE=(8, 16, 32, 64, 128), STRADDLE_THRESH=0, OCTAVE=2.0, USE_FPN=True, FREEZE=False, FORCE_BOXES=False)
    m.ATSS = ns(TOPK=9, REG_LOSS_WEIGHT=2.0, INFERENCE_TH=0.05, PRE_NMS_TOP_N=100, NMS_TH=0.6, DETECTIONS_PER_IMG=20, NUM_CLASSES=2,
                INFERENCE_TH_TRAIN=0.0, PRE_NMS_TOP_N_TRAIN=3000, POST_NMS_TOP_N_TRAIN=1000)
    m.DYHEAD.SCORE_AGG = "MEAN"
    m.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER = False
    m.LANGUAGE_BACKBONE.FREEZE = False
    m.LANGUAGE_BACKBONE.PAD_MAX = True
    m.LANGUAGE_BACKBONE.MASK_SPECIAL = False
    m.RPN_ONLY, m.RPN_ARCHITECTURE, m.LINEAR_PROB = True, "VLDYHEAD", False
    cfg.TEST = ns(USE_MULTISCALE=False, MDETR_STYLE_AGGREGATE_CLASS_NUM=4)
    cfg.DATASETS = ns(ONE_HOT=False)
    for path, v in over.items():
        node = cfg
        *parents, leaf = path.split(".")
        for p in parents:
            node = getattr(node, p)
        setattr(node, leaf, v)
    return cfg
