"""Cases and plain-torch restatement of grounding training (fiber_amd/modules/grounding_train.py, csrc/atss.hip).

assign_torch and losses_torch are the device-independent yardstick: ATSS assignment (per level the k_l = min(TOPK, A_l) nearest anchor
centres, IoU threshold mean + unbiased std, the 0.01 centre test, highest IoU among several gts) and the GIoU / centerness / BCE sums in plain
torch at any dtype on any device.  tests/test_atss_compare_host.py holds them against fixtures the reference's own ATSSLossComputation
produced (tools/gen_atss_golden.py: inputs by name from here, the fixtures hold outputs only); tests/test_hip_atss.py holds the kernels
against their fp64 evaluation.

All cases use the 160 x 224 image of the detect cases with strides (8, 16, 32, 64, 128): 560 / 140 / 35 / 12 / 4 anchors, A = 751; the last
level has k_l = 4 < TOPK, sum k_l = 40.
  atss_small  B = 2, gts 3 and 1.
  atss_edge   B = 3: an image without gts; an image whose only gt is 5 x 5 pixels between anchor centres (gts but no positive); an image
              with 7 heavily overlapping gts (anchors positive for several); one regression prediction beyond the log(1000/16) clamp and one
              inverted predicted box (x2 < x1), both on assigned anchors.
  atss_many   B = 1, 70 gts (past a wave's 64 lanes), Gmax = 72 with NaN boxes in the padding rows.
  atss_ties   OUR tie rules (the reference's topk order on ties is unspecified; checked against the restatement only): a gt centred on
              a shared corner of four level-0 cells (4 anchors at sqrt(32), then 8 at sqrt(160) across the cut at 9: lowest anchor
              indices win) and two identical gt boxes (the lower gt index wins).

Float bound, per element: |got - ref| <= K * 2^-23 * magnitude with the magnitudes of reg_mag / ctr_mag / the sums of |terms| below.  The
constants are 4 x what the reference's own fp32 evaluation needs against fp64 on the same inputs (tools/gen_atss_golden.py measures it on
the CPU), with a floor of 8: the factor covers the device's exp / log / sqrt and the different fixed summation order.
"""
import math
import types

import numpy as np
import torch

from oracle import detgen

T = 256
TOPK = 9
CLIP = math.log(1000.0 / 16)
EPS = 2.0 ** -23
SIZES = [(20, 28), (10, 14), (5, 7), (3, 4), (2, 2)]
STRIDES = (8, 16, 32, 64, 128)
ANCHOR_SIZES = (64, 128, 256, 512, 1024)
IMAGE = (224, 160)                                          # (w, h)
A_TOTAL = sum(h * w for h, w in SIZES)
K_TOTAL = sum(min(TOPK, h * w) for h, w in SIZES)
REG_LOSS_WEIGHT = 2.0

# needed by the reference's fp32 evaluation against fp64 (tools/gen_atss_golden.py prints them) -> 4 x, floor 8
MEASURED = {"K_REG": 0.49, "K_CTR": 0.17, "K_SUM": 1.43, "K_GRAD": 18.84}
CONST = {k: max(8.0, 4.0 * v) for k, v in MEASURED.items()}
# the margins a fixture must have for its discrete outputs to be comparable (conditions, not measurements)
MARGINS = {"cut_gap": 1e-4, "iou_vs_thresh": 1e-5, "centre_vs_001": 1e-4, "best_vs_second": 1e-5, "kink": 1e-4}

CASES = {
    "atss_small": dict(B=2, gts=[3, 1], gmax=3, seed=0),
    "atss_edge": dict(B=3, gts=[0, 1, 7], gmax=8, seed=0),
    "atss_many": dict(B=1, gts=[70], gmax=72, seed=1),
    "atss_ties": dict(B=1, gts=[3], gmax=4, seed=0),
}
GOLDEN = ("atss_small", "atss_edge", "atss_many")           # the cases the reference is decisive on


def cfg():
    """The configuration nodes make_anchor_generator_complex and ATSSLossComputation read."""
    ns = types.SimpleNamespace
    return ns(MODEL=ns(RPN=ns(ANCHOR_SIZES=ANCHOR_SIZES, ASPECT_RATIOS=(1.0,), ANCHOR_STRIDE=STRIDES, STRADDLE_THRESH=0, OCTAVE=2.0,
                              SCALES_PER_OCTAVE=1, USE_FPN=True),
                       ATSS=ns(TOPK=TOPK, REG_LOSS_WEIGHT=REG_LOSS_WEIGHT), RPN_ONLY=True))


def anchors():
    from fiber_amd.modules.grounding_inference import make_anchor_generator_complex
    return make_anchor_generator_complex(cfg()).grid_anchors(SIZES)


def _boxes(g, n, lo=12.0, hi=150.0):
    w, h = g.uniform(lo, hi, n), g.uniform(lo, hi * 0.7, n)
    x, y = g.uniform(0, IMAGE[0] - 1 - w), g.uniform(0, IMAGE[1] - 1 - h)
    return np.stack([x, y, x + w, y + h], axis=1).astype(np.float32)


def inputs(case, seed=None):
    """-> dict(boxes [list of [G_b, 4]], labels [list of [G_b] int64], pmap uint8 [sum G_b, T]; bbox_reg [B, 4, H, W] and centerness
    [B, 1, H, W] per level; fp32 CPU), seeded by name."""
    c = CASES[case]
    g = detgen._rng("atss:" + case, c["seed"] if seed is None else seed)
    B = c["B"]
    boxes = [torch.from_numpy(_boxes(g, n)) for n in c["gts"]]
    if case == "atss_edge":
        # 5 x 5 pixels: its x range holds only the level-1 centre 39.5, its y range only the level-2 centre 47.5: no anchor centre inside
        boxes[1] = torch.tensor([[36.4, 44.3, 40.4, 48.3]])
        base = _boxes(g, 1, 60.0, 110.0)[0]
        jit = g.uniform(-9.0, 9.0, (7, 4)).astype(np.float32)
        boxes[2] = torch.from_numpy(base[None, :] + jit)
    if case == "atss_ties":
        boxes[0] = torch.tensor([[16.0, 20.0, 79.0, 75.0], [100.0, 30.0, 180.0, 120.0], [100.0, 30.0, 180.0, 120.0]])
    labels = [torch.from_numpy(g.integers(1, 80, size=n)) for n in c["gts"]]
    n = sum(c["gts"])
    pm = (g.random((n, T)) < 0.02).astype(np.uint8)
    pm[:, T - 1] = 0
    pm[np.arange(n), g.integers(0, T - 1, size=n)] = 1                           # every gt has a token of its own
    r = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))    # noqa: E731
    out = dict(boxes=boxes, labels=labels, pmap=torch.from_numpy(pm), bbox_reg=[], centerness=[])
    for (h, w) in SIZES:
        out["bbox_reg"].append(r(B, 4, h, w) * torch.tensor([3.0, 3.0, 1.5, 1.5]).view(1, 4, 1, 1))
        out["centerness"].append(0.5 + 1.5 * r(B, 1, h, w))
    return out


def packed(case, x=None, device="cpu"):
    """-> GroundingTargets of the case (atss_many: NaN boxes in the padding rows)"""
    from fiber_amd.modules.grounding_train import pack_targets
    x = inputs(case) if x is None else x
    t = pack_targets(x["boxes"], x["labels"], x["pmap"], gmax=CASES[case]["gmax"])
    if case == "atss_many":
        for b, n in enumerate(CASES[case]["gts"]):
            t.boxes[b, n:] = float("nan")
    return t.to(device)


def mark_edge(case, x, matched):
    """atss_edge: put one regression prediction beyond the clamp and one inverted box on ASSIGNED anchors of level 0 (matched: int [B, A])."""
    if case != "atss_edge":
        return x
    pos = (matched[2, :SIZES[0][0] * SIZES[0][1]] >= 0).nonzero().flatten().tolist()
    assert len(pos) >= 2, "atss_edge: image 2 needs two assigned level-0 anchors"
    W = SIZES[0][1]
    reg = x["bbox_reg"][0]
    reg[2, 2, pos[0] // W, pos[0] % W] = 30.0               # dw = 6 > log(1000 / 16)
    reg[2, 2, pos[1] // W, pos[1] % W] = -40.0              # width exp(-8) * 64 << 1: x2 = x1 + w - 1 < x1
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def iou_plus_one(an, gt):
    """boxlist_iou (boxlist_ops.py:116-130): an [A, 4], gt [G, 4] -> [A, G]"""
    a1 = (an[:, 2] - an[:, 0] + 1) * (an[:, 3] - an[:, 1] + 1)
    a2 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    lt = torch.max(an[:, None, :2], gt[:, :2])
    rb = torch.min(an[:, None, 2:], gt[:, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (a1[:, None] + a2 - inter)


def encode(gt, an):
    """BoxCoder.encode (box_coder.py:32-50), weights (10, 10, 5, 5) -> (codes [N, 4], magnitudes [N, 4] for the float bound)"""
    ew, eh = an[:, 2] - an[:, 0] + 1, an[:, 3] - an[:, 1] + 1
    ex, ey = an[:, 0] + 0.5 * ew, an[:, 1] + 0.5 * eh
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gx, gy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    code = torch.stack((10.0 * (gx - ex) / ew, 10.0 * (gy - ey) / eh, 5.0 * torch.log(gw / ew), 5.0 * torch.log(gh / eh)), dim=1)
    mag = torch.stack((10.0 * (gx.abs() + ex.abs()) / ew, 10.0 * (gy.abs() + ey.abs()) / eh, 5.0 + code[:, 2].abs(), 5.0 + code[:, 3].abs()), dim=1)
    return code, mag


def assign_torch(anchors_per_level, targets, topk=TOPK, dtype=torch.float64):
    """targets: GroundingTargets (any device).  -> dict: matched int32 [B, A], labels int32, reg_targets [B, A, 4], token_targets uint8
    [B, A, T], num_pos int32 [B], reg_mag [B, A, 4]; cand_idx / cand_iou [B, Gmax, K] (live rows), and the decisiveness margins."""
    dev = targets.boxes.device
    an = torch.cat([a.to(dev) for a in anchors_per_level]).to(dtype)
    A = an.shape[0]
    B, G = targets.labels.shape
    sizes = [a.shape[0] for a in anchors_per_level]
    K = sum(min(topk, n) for n in sizes)
    acx, acy = (an[:, 2] + an[:, 0]) / 2.0, (an[:, 3] + an[:, 1]) / 2.0
    out = dict(matched=torch.full((B, A), -1, dtype=torch.int32, device=dev), labels=torch.zeros((B, A), dtype=torch.int32, device=dev),
               reg_targets=torch.zeros((B, A, 4), dtype=dtype, device=dev), reg_mag=torch.ones((B, A, 4), dtype=dtype, device=dev),
               token_targets=torch.zeros((B, A, T), dtype=torch.uint8, device=dev), num_pos=torch.zeros((B,), dtype=torch.int32, device=dev),
               cand_idx=torch.full((B, G, K), -1, dtype=torch.int32, device=dev), cand_iou=torch.zeros((B, G, K), dtype=dtype, device=dev))
    out["token_targets"][:, :, T - 1] = 1
    m = dict(cut_gap=math.inf, iou_vs_thresh=math.inf, centre_vs_001=math.inf, best_vs_second=math.inf)
    ngt = targets.num_gt.tolist()
    for b in range(B):
        n = ngt[b]
        if n == 0:
            continue
        gt = targets.boxes[b, :n].to(dtype)
        iou = iou_plus_one(an, gt)                                               # [A, n]
        gcx, gcy = (gt[:, 2] + gt[:, 0]) / 2.0, (gt[:, 3] + gt[:, 1]) / 2.0
        dist = ((acx[:, None] - gcx[None, :]).pow(2) + (acy[:, None] - gcy[None, :]).pow(2)).sqrt()
        cand, lo = [], 0
        for s in sizes:
            k = min(topk, s)
            d, order = torch.sort(dist[lo:lo + s], dim=0, stable=True)           # stable: equal distances to the lowest anchor index
            cand.append(order[:k] + lo)
            if k < s:
                m["cut_gap"] = min(m["cut_gap"], float((d[k] - d[k - 1]).min()))
            lo += s
        cand = torch.cat(cand, dim=0)                                            # [K, n]
        ci = torch.gather(iou, 0, cand)
        thr = ci.mean(0) + ci.std(0)
        ctr_min = torch.stack([acx[cand] - gt[:, 0], acy[cand] - gt[:, 1], gt[:, 2] - acx[cand], gt[:, 3] - acy[cand]], dim=0).min(0)[0]
        pos = (ci >= thr[None, :]) & (ctr_min > 0.01)
        m["iou_vs_thresh"] = min(m["iou_vs_thresh"], float((ci - thr[None, :]).abs().min()))
        m["centre_vs_001"] = min(m["centre_vs_001"], float((ctr_min - 0.01).abs().min()))
        inf = torch.full((A, n), -1.0, dtype=dtype, device=dev)
        cols = torch.arange(n, device=dev)[None, :].expand(K, n)
        inf[cand[pos], cols[pos]] = ci[pos]
        best, arg = inf.max(dim=1)
        arg = (inf == best[:, None]).to(torch.int8).argmax(dim=1)                # equal IoU to the lowest gt index
        hit = best >= 0
        multi = (inf >= 0).sum(1) > 1
        if bool(multi.any()):
            top2 = torch.topk(inf[multi], 2, dim=1)[0]
            m["best_vs_second"] = min(m["best_vs_second"], float((top2[:, 0] - top2[:, 1]).min()))
        out["multi_%d" % b] = int(multi.sum())
        code, mag = encode(gt[arg], an)
        out["matched"][b] = torch.where(hit, arg, torch.full_like(arg, -1)).to(torch.int32)
        out["labels"][b] = torch.where(hit, targets.labels[b, :n].long()[arg], torch.zeros_like(arg)).to(torch.int32)
        out["reg_targets"][b] = torch.where(hit[:, None], code, torch.zeros_like(code))
        out["reg_mag"][b] = torch.where(hit[:, None], mag, torch.ones_like(mag))
        out["token_targets"][b] = torch.where(hit[:, None], targets.positive_map[b, :n][arg], out["token_targets"][b])
        out["num_pos"][b] = int((out["labels"][b] > 0).sum())
        out["cand_idx"][b, :n], out["cand_iou"][b, :n] = cand.t().to(torch.int32), ci.t()
    out["margins"] = m
    return out


def decode(code, an):
    """BoxCoder.decode (box_coder.py:64-93) on [N, 4] -> (x1, y1, x2, y2, pw, ph)"""
    w, h = an[:, 2] - an[:, 0] + 1, an[:, 3] - an[:, 1] + 1
    cx, cy = an[:, 0] + 0.5 * w, an[:, 1] + 0.5 * h
    dx, dy = code[:, 0] / 10.0, code[:, 1] / 10.0
    dw, dh = torch.clamp(code[:, 2] / 5.0, max=CLIP), torch.clamp(code[:, 3] / 5.0, max=CLIP)
    px, py, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    return px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw - 1, py + 0.5 * ph - 1, pw, ph


def flatten_levels(levels, ch):
    """[B, ch, H, W] per level -> [B, A, ch] in the anchors' order (concat_box_prediction_layers for one anchor per location)"""
    return torch.cat([t.reshape(t.shape[0], ch, -1).permute(0, 2, 1) for t in levels], dim=1)


def losses_torch(bbox_reg, centerness, anchors_per_level, labels, reg_targets, dtype=torch.float64, grads=None):
    """GIoULoss, compute_centerness_targets and BCEWithLogits(sum) over labels > 0 (loss.py:583-624, :829-844, :1237-1254), dense and
    masked.  -> dict: sums [3] (sum w (1 - giou), sum w, sum BCE), sums_abs [3] (sums of |terms|), w [B, A], ctr_mag [B, A], kink (the
    least distance of a max / min / clamp argument pair from its kink over the assigned anchors); with grads = (g0, g1, g2): d_bbox_reg /
    d_centerness per level by autograd and grad_mag [B, A, 4], the magnitude of the per-element gradient bound."""
    dev = labels.device
    an = torch.cat([a.to(dev) for a in anchors_per_level]).to(dtype)
    regs = [t.detach().to(dtype).requires_grad_(grads is not None) for t in bbox_reg]
    ctrs = [t.detach().to(dtype).requires_grad_(grads is not None) for t in centerness]
    B, A = labels.shape
    pos = labels > 0
    anb = an[None].expand(B, A, 4)[pos]
    code, z = flatten_levels(regs, 4)[pos], flatten_levels(ctrs, 1)[pos][:, 0]
    tg = reg_targets.to(dtype)[pos]
    tx1, ty1, tx2, ty2, tw, th = decode(tg, anb)
    acx, acy = (anb[:, 2] + anb[:, 0]) / 2, (anb[:, 3] + anb[:, 1]) / 2
    l, t, r, b = acx - tx1, acy - ty1, tx2 - acx, ty2 - acy
    w = torch.sqrt((torch.min(l, r) / torch.max(l, r)) * (torch.min(t, b) / torch.max(t, b)))
    X, Y = acx.abs() + (tx1 + tx2).abs() / 2 + tw, acy.abs() + (ty1 + ty2).abs() / 2 + th
    wmag = w * (1 + X / torch.min(l, r).abs() + Y / torch.min(t, b).abs())
    px1, py1, px2r, py2r, pw, ph = decode(code, anb)
    px2, py2 = torch.max(px1, px2r), torch.max(py1, py2r)
    parea = (px2 - px1) * (py2 - py1)
    tarea = (tx2 - tx1) * (ty2 - ty1)
    ix1, iy1, ix2, iy2 = torch.max(px1, tx1), torch.max(py1, ty1), torch.min(px2, tx2), torch.min(py2, ty2)
    mask = (iy2 > iy1) & (ix2 > ix1)
    inter = torch.where(mask, (ix2 - ix1) * (iy2 - iy1), torch.zeros_like(ix1))
    ex1, ey1, ex2, ey2 = torch.min(px1, tx1), torch.min(py1, ty1), torch.max(px2, tx2), torch.max(py2, ty2)
    earea = (ex2 - ex1) * (ey2 - ey1) + 1e-7
    union = parea + tarea - inter + 1e-7
    giou = inter / union - (earea - union) / earea
    terms = (w * (1 - giou), w, torch.nn.functional.binary_cross_entropy_with_logits(z, w, reduction="none"))
    out = dict(sums=torch.stack([x.sum() for x in terms]), sums_abs=torch.stack([x.detach().abs().sum() for x in terms]))

    def full(v):
        o = torch.zeros((B, A) + v.shape[1:], dtype=dtype, device=dev)
        o[pos] = v.detach()
        return o
    out["w"], out["ctr_mag"] = full(w), full(wmag)
    # (an inverted axis has px2 = px1 exactly, hence ix2 - ix1 = 0 EXACTLY at any precision: a structural zero of the strict test, no kink)
    upx, upy = px2r > px1, py2r > py1
    pairs = [px1 - px2r, py1 - py2r, px1 - tx1, py1 - ty1, px2 - tx2, py2 - ty2, (ix2 - ix1)[upx], (iy2 - iy1)[upy], code[:, 2] / 5.0 - CLIP,
             code[:, 3] / 5.0 - CLIP, l - r, t - b]
    out["kink"] = min((float(p.detach().abs().min()) for p in pairs if p.numel()), default=math.inf) if int(pos.sum()) else math.inf
    if grads is not None:
        g = torch.as_tensor(grads, dtype=dtype, device=dev)
        if int(pos.sum()):
            (out["sums"] * g).sum().backward()
        out["d_bbox_reg"], out["d_centerness"] = [t.grad if t.grad is not None else torch.zeros_like(t) for t in regs], \
            [t.grad if t.grad is not None else torch.zeros_like(t) for t in ctrs]
        # every d giou / d corner is bounded by a few times extent * (1 / U + 1 / E); the chain to the codes multiplies by the anchor or
        # the decoded extent over the coder's weight
        aw, ah = anb[:, 2] - anb[:, 0] + 1, anb[:, 3] - anb[:, 1] + 1
        s = (g[0].abs() * w * (1 / union + 1 / earea)).detach()
        eh, ew = (ey2 - ey1).detach(), (ex2 - ex1).detach()
        gm = torch.stack((s * eh * aw / 10, s * ew * ah / 10, s * eh * pw.detach() / 10, s * ew * ph.detach() / 10), dim=1)
        out["grad_mag"] = full(gm)
        out["ctr_grad_mag"] = full(g[2].abs() * (1 + w.detach()))
    out["sums"] = out["sums"].detach()
    return out


def need(got, ref, mag):
    """the constant K an element-wise comparison needs: max |got - ref| / (2^-23 * magnitude)"""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref.double()).abs() / (EPS * mag.double().clamp_min(1e-300))).max())


assert A_TOTAL == 751 and K_TOTAL == 40
