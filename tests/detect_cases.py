"""Cases and plain-torch restatement of grounding inference (fiber_amd/modules/grounding_inference.py, csrc/detect.hip).

postprocess_torch is the device-independent yardstick: the fixed-shape pipeline (dense scores with -1 padding, per-level top-k with the fixed
k_l, decode + clip, stable descending sort, label-aware greedy NMS with the +1 IoU of ml_nms.cu's devIoU and strict >, the first D survivors)
in plain torch at any dtype on any device.  tests/test_detect_compare_host.py holds it against fixtures the reference's own ATSSPostProcessor
produced (tools/gen_detect_golden.py: inputs by name from here, the fixtures hold outputs only); tests/test_hip_detect.py holds the kernels
against its fp64 evaluation.

Cases (the seeds are those tools/gen_detect_golden.py found to satisfy the decisiveness margins it asserts and stores):
  detect_small   B = 2, levels (20,28) (10,14) (5,7) = 735 anchors, strides 8/16/32, images (224,160) and (200,150) as (w, h); C = 6 with
                 overlapping token sets, one single-token class and one empty class; MEAN, thresh 0.05, top-n 200 (N = 600), NMS 0.6, D = 100.
                 The cut bites on levels 0 and 1; level 2 has 35 x 5 = 175 live entries < 200, so its slice ends in padding.
  detect_refexp  same geometry; v2 mapping with num_class 100, MAX, thresh 0.0.  List-valued entries: the reference's MAX branch of
                 convert_grounding_to_od_logits_v2 does not wrap an int entry (inference.py:787-789), so int entries are in detect_edge.
                 top-n 120 (N = 360), lowered from the configs' 3000: the IoU margin has to hold on EVERY same-label pair, and their
                 number grows with N^2 (see the generator).  No token is shared: under MAX a shared token gives two labels of one anchor the
                 same score exactly, which no margin survives.
  detect_edge    B = 1, one level (3,5), v2 mapping with int-valued entries and MEAN; N = 60 (no multiple of 64), fewer than D survivors,
                 one box decoded fully outside the image, one dw above the log(1000/16) clamp.

Float bound (per element, the project's form constant x 2^-23 x magnitude; needs measured on MI355X against the fp64 evaluation, see
profiles/ground_inference.md; the bound is 2 x the need rounded up to a power of two):
  scores  |got - ref| <= K_SCORE * 2^-23 * max(|ref|, tiny)
  boxes   |got - ref| <= K_BOX * 2^-23 * (|ctr| + pred_w)   per axis, ctr / pred_w the fp64 decoded centre and extent before clipping
"""
import math
import types

import numpy as np
import torch

from oracle import detgen

T = 256
CLIP = math.log(1000.0 / 16)
CONST = {
    "K_SCORE": 8.0,    # one-exp sigmoid (v_exp, v_rcp) x 2, the fold over a class's tokens, the product, the sqrt (3.47: dense scores, detect_refexp level 0)
    "K_BOX": 2.0,      # fp32 decode in the reference's operation order, expf (0.83: detect_small level 0)
}
EPS = 2.0 ** -23
SRC_A_SHIFT, SRC_L_SHIFT = 10, 28

GEOM3 = dict(sizes=[(20, 28), (10, 14), (5, 7)], strides=(8, 16, 32), anchor_sizes=(64, 128, 256))
CASES = {
    "detect_small": dict(B=2, image_sizes=[(224, 160), (200, 150)], C=6, v2=False, agg="MEAN", thresh=0.05, top_n=200, nms=0.6, D=100,
                         positive_map={1: [3, 4, 5], 2: [5, 6], 3: [17], 4: [30, 31, 32, 33, 200], 6: [4, 31, 90]}, seed=1, **GEOM3),
    "detect_refexp": dict(B=2, image_sizes=[(224, 160), (200, 150)], C=100, v2=True, agg="MAX", thresh=0.0, top_n=120, nms=0.6, D=100,
                          positive_map={1: [7], 2: [8, 9, 10], 40: [11, 21], 100: [255]}, seed=2, **GEOM3),
    "detect_edge": dict(B=1, image_sizes=[(160, 96)], C=4, v2=True, agg="MEAN", thresh=0.05, top_n=100, nms=0.6, D=100,
                        positive_map={1: 3, 2: 10, 4: 200}, seed=0, sizes=[(3, 5)], strides=(32,), anchor_sizes=(64,)),
}
# the margins a fixture must have for its discrete outputs to be comparable (conditions, not measurements)
MARGINS = {"agg_vs_thresh": 1e-5, "cut_gap": 1e-5, "sorted_gap": 1e-6, "iou_vs_nms": 1e-4}


def cfg_for(case):
    """The configuration nodes make_anchor_generator_complex / make_atss_postprocessor read."""
    ns = types.SimpleNamespace
    c = CASES[case] if isinstance(case, str) else case
    return ns(MODEL=ns(RPN=ns(ANCHOR_SIZES=c["anchor_sizes"], ASPECT_RATIOS=(1.0,), ANCHOR_STRIDE=c["strides"], STRADDLE_THRESH=0, OCTAVE=2.0,
                              SCALES_PER_OCTAVE=1, USE_FPN=True),
                       ATSS=ns(INFERENCE_TH=c["thresh"], PRE_NMS_TOP_N=c["top_n"], NMS_TH=c["nms"], DETECTIONS_PER_IMG=c["D"], NUM_CLASSES=c["C"] + 1,
                               INFERENCE_TH_TRAIN=0.0, PRE_NMS_TOP_N_TRAIN=3000, POST_NMS_TOP_N_TRAIN=1000),
                       DYHEAD=ns(SCORE_AGG=c["agg"])),
              TEST=ns(USE_MULTISCALE=False, MDETR_STYLE_AGGREGATE_CLASS_NUM=c["C"] if c["v2"] else -1))


def inputs(case, seed=None):
    """-> dict(logits [B, A_l, T], bbox_reg [B, 4, H, W], centerness [B, 1, H, W] per level; fp32 CPU), seeded by name."""
    c = CASES[case]
    g = detgen._rng("detect:" + case, c["seed"] if seed is None else seed)
    B = c["B"]
    r = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))    # noqa: E731
    out = dict(logits=[], bbox_reg=[], centerness=[])
    for (h, w) in c["sizes"]:
        A = h * w
        out["logits"].append(-2.2 + 1.3 * r(B, A, 1) + 1.1 * r(B, A, T))
        out["bbox_reg"].append(r(B, 4, h, w) * torch.tensor([6.0, 6.0, 3.0, 3.0]).view(1, 4, 1, 1))
        out["centerness"].append(0.5 + 1.5 * r(B, 1, h, w))
    if case == "detect_edge":
        lg, reg = out["logits"][0], out["bbox_reg"][0]
        lg[0, 4, :], lg[0, 7, :] = 2.0 + 0.1 * r(T), 1.5 + 0.1 * r(T)           # both anchors are candidates for every live class
        reg[0, 0, 0, 4] = 100.0                                                  # dx / 10 * w = 10 widths to the right: outside, clipped to the edge
        reg[0, 2, 1, 2] = 30.0                                                   # anchor 7: dw = 6 > log(1000 / 16)
    return out


def csr(positive_map, C, v2=False):
    from fiber_amd.modules.grounding_inference import positive_map_to_csr
    return positive_map_to_csr(positive_map, C, v2)


def anchors_for(case):
    from fiber_amd.modules.grounding_inference import make_anchor_generator_complex
    c = CASES[case] if isinstance(case, str) else case
    return make_anchor_generator_complex(cfg_for(c)).grid_anchors(c["sizes"])


def level_k(top_n, A, C):
    return min(int(top_n), A * C)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def dense_scores(logits, ctr, positive_map, C, agg, thresh, dtype=torch.float64, after_ctr=False):
    """-> (dense [B, A, C]: agg * sigmoid(ctr) where agg > thresh else -1, agg [B, A, C]).  after_ctr: the MUTATION that tests the product."""
    B, A, _ = logits.shape
    p = torch.sigmoid(logits.to(dtype))
    a = torch.zeros((B, A, C), dtype=dtype, device=logits.device)
    for label, toks in positive_map.items():
        toks = torch.as_tensor([toks] if isinstance(toks, int) else list(toks), dtype=torch.long, device=logits.device)
        sel = p[:, :, toks]
        a[:, :, int(label) - 1] = sel.mean(-1) if agg == "MEAN" else sel.max(-1)[0]
    s = a * torch.sigmoid(ctr.to(dtype).reshape(B, A))[:, :, None]
    cand = (s if after_ctr else a) > thresh
    return torch.where(cand, s, torch.full_like(s, -1.0)), a


def decode(val, flat, reg, anchors, sizes, C, level, dtype=torch.float64, min_size=0.0):
    """val / flat [B, k] -> boxes [B, k, 4], scores, labels, source, mag [B, k, 2] (|ctr| + pred extent per axis, for the box bound)"""
    B, k = val.shape
    A = anchors.shape[0]
    a, c = torch.div(flat, C, rounding_mode="floor"), flat % C
    r = reg.to(dtype).reshape(B, 4, A).gather(2, a[:, None, :].expand(-1, 4, -1))          # [B, 4, k]
    an = anchors.to(dtype)[a]                                                             # [B, k, 4]
    w, h = an[..., 2] - an[..., 0] + 1, an[..., 3] - an[..., 1] + 1
    cx, cy = an[..., 0] + 0.5 * w, an[..., 1] + 0.5 * h
    dx, dy = r[:, 0] / 10.0, r[:, 1] / 10.0
    dw, dh = torch.clamp(r[:, 2] / 5.0, max=CLIP), torch.clamp(r[:, 3] / 5.0, max=CLIP)
    px, py, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    iw, ih = (sizes[:, 0].to(dtype) - 1)[:, None], (sizes[:, 1].to(dtype) - 1)[:, None]
    zero = torch.zeros((), dtype=dtype, device=val.device)
    box = torch.stack((torch.minimum(torch.maximum(px - 0.5 * pw, zero), iw), torch.minimum(torch.maximum(py - 0.5 * ph, zero), ih),
                       torch.minimum(torch.maximum(px + 0.5 * pw - 1, zero), iw), torch.minimum(torch.maximum(py + 0.5 * ph - 1, zero), ih)), dim=-1)
    live = val >= 0
    big = (box[..., 2] - box[..., 0] + 1 >= min_size) & (box[..., 3] - box[..., 1] + 1 >= min_size)
    sc = torch.where(live & big, torch.sqrt(val.to(dtype).clamp_min(0)), torch.full_like(val, -1.0, dtype=dtype))
    lab = torch.where(live, c + 1, torch.zeros_like(c)).to(torch.int32)
    src = torch.where(live, (level << SRC_L_SHIFT) | (a << SRC_A_SHIFT) | c, torch.full_like(c, -1)).to(torch.int32)
    box = torch.where(live[..., None], box, torch.zeros_like(box))
    mag = torch.stack((px.abs() + pw, py.abs() + ph), dim=-1)
    return box, sc, lab, src, mag


def iou_matrix(boxes, plus_one=True):
    """[B, N, 4] -> [B, N, N] in devIoU's operation order (ml_nms.cu:15-26)"""
    one = 1.0 if plus_one else 0.0
    a, b = boxes[:, :, None, :], boxes[:, None, :, :]
    wd = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0]) + one).clamp_min(0)
    ht = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1]) + one).clamp_min(0)
    inter = wd * ht
    area = (boxes[..., 2] - boxes[..., 0] + one) * (boxes[..., 3] - boxes[..., 1] + one)
    return inter / (area[:, :, None] + area[:, None, :] - inter)


def suppression(boxes, scores, labels, nms, ge=False, plus_one=True, label_blind=False):
    """bool [B, N, N]: row i suppresses column j (j > i, same label, IoU > nms, both live)"""
    N = scores.shape[1]
    iou = iou_matrix(boxes, plus_one)
    over = (iou >= nms) if ge else (iou > nms)
    same = torch.ones_like(over) if label_blind else labels[:, :, None] == labels[:, None, :]
    live = scores >= 0
    upper = torch.triu(torch.ones((N, N), dtype=torch.bool, device=boxes.device), diagonal=1)
    return over & same & live[:, :, None] & live[:, None, :] & upper


def mask_words(sup):
    """bool [B, N, N] -> int64 [B, N, ceil(N / 64)] (the mask kernel's layout; bit j % 64 of word j / 64)"""
    B, N, _ = sup.shape
    NB = (N + 63) // 64
    pad = torch.zeros((B, N, NB * 64), dtype=torch.int64, device=sup.device)
    pad[:, :, :N] = sup.to(torch.int64)
    bits = pad.view(B, N, NB, 64)
    w = torch.zeros((B, N, NB), dtype=torch.int64, device=sup.device)
    for j in range(64):
        v = 1 << j if j < 63 else -(1 << 63)
        w |= bits[..., j] * v
    return w


def greedy_keep(sup, scores, D):
    """The walk of ml_nms.cu:122-140 on device tensors, stopping at D kept -> keep bool [B, N]"""
    B, N, _ = sup.shape
    removed = scores < 0
    keep = torch.zeros_like(removed)
    count = torch.zeros((B,), dtype=torch.long, device=scores.device)
    for i in range(N):
        k = ~removed[:, i] & (count < D)
        keep[:, i] = k
        count += k
        removed |= sup[:, i] & k[:, None]
    return keep


def select(boxes, scores, labels, source, keep, D):
    """-> fixed-size (boxes [B, D, 4], scores, labels, source, count), padding as the select kernel writes it"""
    B, N = scores.shape
    count = keep.sum(1)
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True)[1][:, :D]              # kept first, in their (score) order
    if order.shape[1] < D:
        order = torch.cat([order, order.new_zeros((B, D - order.shape[1]))], 1)
    live = torch.arange(D, device=scores.device)[None, :] < count[:, None]
    ob = torch.where(live[..., None], torch.gather(boxes, 1, order[..., None].expand(-1, -1, 4)), torch.zeros((), dtype=boxes.dtype, device=boxes.device))
    osc = torch.where(live, torch.gather(scores, 1, order), torch.full((), -1.0, dtype=scores.dtype, device=scores.device))
    ol = torch.where(live, torch.gather(labels, 1, order), torch.zeros((), dtype=labels.dtype, device=labels.device))
    osr = torch.where(live, torch.gather(source, 1, order), torch.full((), -1, dtype=source.dtype, device=source.device))
    return ob, osc, ol, osr, count.to(torch.int32)


def postprocess_torch(logits, bbox_reg, centerness, anchors, image_sizes, positive_map, C, agg, thresh, top_n, nms, D, dtype=torch.float64,
                      ge=False, plus_one=True, after_ctr=False, label_blind=False, min_size=0.0):
    """The whole pipeline.  image_sizes: [B, 2] tensor or list of (w, h).  -> dict: boxes / scores / labels / source / count (fixed size D) and
    the intermediates (agg, dense, topk values per level; cand_* the sorted candidates, mag their box magnitudes, sup, keep)."""
    dev = logits[0].device
    sizes = torch.as_tensor(image_sizes, dtype=dtype, device=dev) if not torch.is_tensor(image_sizes) else image_sizes.to(device=dev, dtype=dtype)
    out = dict(agg=[], dense=[], topk=[], rest=[])
    parts = []
    for l, (lg, reg, ctr, anc) in enumerate(zip(logits, bbox_reg, centerness, anchors)):
        B, A, _ = lg.shape
        dense, a = dense_scores(lg, ctr, positive_map, C, agg, thresh, dtype, after_ctr)
        k = level_k(top_n, A, C)
        flatd = dense.reshape(B, -1)
        val, flat = torch.topk(flatd, k, dim=1)
        out["agg"].append(a), out["dense"].append(dense), out["topk"].append(val)
        if k < flatd.shape[1]:                                  # the best entry the cut leaves out (for the gap across the cut)
            out["rest"].append(torch.topk(flatd, k + 1, dim=1)[0][:, k])
        else:
            out["rest"].append(torch.full((B,), -1.0, dtype=dtype, device=dev))
        parts.append(decode(val, flat, reg, anc.to(dev), sizes, C, l, dtype, min_size))
    boxes, scores, labels, source, mag = (torch.cat([p[i] for p in parts], dim=1) for i in range(5))
    scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
    boxes = torch.gather(boxes, 1, order[..., None].expand(-1, -1, 4))
    mag = torch.gather(mag, 1, order[..., None].expand(-1, -1, 2))
    labels, source = torch.gather(labels, 1, order), torch.gather(source, 1, order)
    sup = suppression(boxes, scores, labels, nms, ge, plus_one, label_blind)
    keep = greedy_keep(sup, scores, D)
    ob, osc, ol, osr, cnt = select(boxes, scores, labels, source, keep, D)
    omag = select(mag.repeat(1, 1, 2), scores, labels, source, keep, D)[0][..., :2]
    out.update(cand_boxes=boxes, cand_scores=scores, cand_labels=labels, cand_source=source, cand_mag=mag, sup=sup, keep=keep,
               boxes=ob, scores=osc, labels=ol, source=osr, count=cnt, mag=omag)
    return out


def run_case(case, dtype=torch.float64, device="cpu", seed=None, **mut):
    c = CASES[case]
    x = inputs(case, seed)
    to = lambda ts: [t.to(device) for t in ts]              # noqa: E731
    return postprocess_torch(to(x["logits"]), to(x["bbox_reg"]), to(x["centerness"]), to(anchors_for(case)), c["image_sizes"], c["positive_map"],
                             c["C"], c["agg"], c["thresh"], c["top_n"], c["nms"], c["D"], dtype=dtype, **mut)


def score_bound(ref, k=None):
    return (CONST["K_SCORE"] if k is None else k) * EPS * ref.abs().clamp_min(2.0 ** -20)


def box_bound(mag, k=None):
    """mag [..., 2] (x, y) -> bound [..., 4]"""
    return (CONST["K_BOX"] if k is None else k) * EPS * torch.cat([mag, mag], dim=-1)


# ---- a large synthetic candidate list for the NMS kernels alone ------------------------------------------------------------------------
BIG = dict(B=2, N=8300, pad=37, labels=3, extent=1400, nms=0.5)


def big_candidates(device="cpu"):
    """Sorted candidates past the select kernel's first bitmap slot: N = 8300 = 129 * 64 + 44 (words 0..129, i.e. slots 0, 1 and 2 of a
    lane), the last 37 padding.  Coordinates are INTEGERS, so with the +1 convention every area and intersection is an exact integer below
    2^24 and IoU = p / q with q < 2^15: fp32 (correctly rounded division) and fp64 agree on `> 0.5` for every pair, exact ties at 1/2
    included (|p / q - 1/2| is 0 or at least 1 / 2q), which strict > must keep.  -> boxes fp32 [B, N, 4], scores, labels, source int32"""
    c = BIG
    g = detgen._rng("detect:big", 0)
    B, N = c["B"], c["N"]
    xy = g.integers(0, c["extent"], size=(B, N, 2))
    wh = g.integers(20, 81, size=(B, N, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh - 1], axis=-1).astype(np.float32))
    scores = torch.from_numpy(np.sort(g.random((B, N)).astype(np.float32) * 0.9 + 0.05, axis=1)[:, ::-1].copy())
    labels = torch.from_numpy(g.integers(1, c["labels"] + 1, size=(B, N)).astype(np.int32))
    source = torch.arange(B * N, dtype=torch.int32).view(B, N)
    scores[:, N - c["pad"]:], labels[:, N - c["pad"]:], source[:, N - c["pad"]:] = -1.0, 0, -1
    boxes[:, N - c["pad"]:] = 0
    return boxes.to(device), scores.to(device), labels.to(device), source.to(device)
